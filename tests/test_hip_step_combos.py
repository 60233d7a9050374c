"""Steps that combine the transport of the style term, a blend or regions, a content-weight map and temporal targets on the
GPU ("Combined steps"): StepEngine on every case of tests/_step_cases.py against the float64
restatement of tests/_step_ref.py -- every scalar and the gradient of EVERY pyramid level --, eager / graph replay / device
draw bit for bit on the cases whose transport term borrows from the separate weighted content entry, the same cases without
x3 panels in a child process, the remd cases without the grouped entry, and the command line with all of it at once.

Run as a script with the argument "x3_off" (a child process under STROTSS_X3=0) this file compares the borrowing cases with
float64 to the same bounds and prints one JSON line."""
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

import _step_cases as C
import _step_ref as R
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
BORROWING = [lb for lb in C.LABELS if C.borrowing(C.ROWS[lb])]
REMD_MAP_TEMPORAL = [lb for lb in C.LABELS if C.ROWS[lb][0] == "remd" and C.ROWS[lb][2] and C.ROWS[lb][3]]


def _engine(lb, deterministic=None):
    """test_hip_transport._engine with content_weight= and temporal= added"""
    from nn import _ops, engine
    from nn.model import VGGParams
    row, P = C.ROWS[lb], C.problem(lb)
    params = VGGParams(P["weights"], '16', None, DEV)
    cfeat = engine.extract_features(params, P["content"].to(DEV))
    sfeats = [engine.extract_features(params, s.to(DEV)) for s in P["styles"]]
    bw = C.blend_of(row)
    targets = []
    for sets in P["s_idx"]:
        ts = [engine.StyleTarget.build(_ops.hypercol_gather(sf, torch.from_numpy(si).to(DEV), False), si.shape[0], 2179)
              for sf, si in zip(sfeats, sets)]
        targets.append(ts[0] if bw is None else engine.StyleBlend(ts, list(bw)))
    c64, s64 = P["content"].double(), P["styles"][0].double()
    init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    tr = C.transport_of(row)
    kw = dict(style_transport=tr[0])
    if tr[0] == "sinkhorn":
        kw.update(sinkhorn_l=tr[1], sinkhorn_iters=tr[2])
    if tr[0] == "sliced":
        assert tr[3] == 0                      # the engine's draw number starts at 0
        kw.update(sliced_projections=tr[1], sliced_seed=tr[2])
    temporal = [engine.TemporalTarget(tg.to(DEV), c.to(DEV), lam) for tg, c, lam in P["temporal"]] or None
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic,
                             content_weight=None if P["wmap"] is None else P["wmap"].to(DEV), temporal=temporal, **kw)


def _indices(lb):
    return [torch.from_numpy(i).to(DEV) for i in C.problem(lb)["idx"]]


def _readout(eng):
    """the engine's losses and gradients shaped like _step_ref.train_step's result"""
    got = dict(eng.losses())
    got["grads"] = [g.detach().cpu().double() for g in eng.gvars]
    return got


_REFS = {}


def reference(lb, eng):
    """the float64 step of case `lb` with the engine's ReLU masks and pool selections (test_hip_engine._oracle_vgg): built
    once per case and trunk routing, shared by the checks that use it, left unchanged"""
    import test_hip_engine as THE
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(C.problem(lb)["weights"], dtype=torch.float64)), eng)
    key = (lb, type(vgg).__name__)
    if key not in _REFS:
        row = C.ROWS[lb]
        _REFS[key] = R.reference_step(C.problem(lb), C.transport_of(row), blend_weights=C.blend_of(row), vgg=vgg)
    return _REFS[key]


def check_against_float64(lb, eng, what="step"):
    """every scalar within TOL_SCALAR relative to max(1, |ref|), every level of the gradient within GRAD_TOL in relative L2;
    each figure printed before anything is asserted"""
    row = C.ROWS[lb]
    ref, got = reference(lb, eng), _readout(eng)
    scalars, levels = R.step_scalars(got, ref, row[0]), R.step_grads(got, ref)
    for k, v in scalars.items():
        print(f"MEASURE {what}:{k} {lb} {v:.3e}")
    for k, v in enumerate(levels):
        print(f"MEASURE {what}:grad_level{k} {lb} {v:.3e}")
    assert got[R.TRANSPORT_KEY[row[0]]] == got["l_remd"] > 0
    assert ("loss_t" in got) == bool(row[3]) and len(got.get("loss_t_terms", [])) == (3 if row[3] == 3 else 0)
    for k, v in scalars.items():
        assert v < R.TOL_SCALAR, (k, v, got.get(k), ref.get(k))
    assert len(levels) == 6
    for k, v in enumerate(levels):
        assert v < R.GRAD_TOL, (k, v)
    ok, sc, gr = R.within_bounds(got, ref, row[0])
    assert ok, (sc, gr)
    P = C.problem(lb)
    if row[3]:                                 # the temporal part is a real share of the step
        share = sum(lam * float(lt) for (_, _, lam), lt in zip(P["temporal"], ref["loss_t_terms"]))
        assert share > 0.05 * float(ref["loss"])
    if row[2]:                                 # some sampled weights are exactly 0
        for r in range(eng.R):
            n = len(P["idx"][r])
            assert int((eng._cw[r][:n] == 0).sum()) > 0 and float(eng._cw[r][:n].max()) > 0
    return max(scalars.values()), levels


# ------------------------------------------------------------------ 1. every case against float64
@pytest.mark.parametrize("lb", C.LABELS)
def test_combined_step_matches_the_float64_restatement(lb):
    from nn import _ops
    row = C.ROWS[lb]
    eng = _engine(lb)
    before = dict(_ops.remd_borrow_stats)
    eng.forward_backward(_indices(lb))
    torch.cuda.synchronize()
    if row[0] == "sliced":                     # one draw per (region, style) call
        assert int(eng._sliced_counter.item()) == {"one": 1, "blend": 2, "regions": 2}[row[1]]
    if row[0] != "remd":                       # the separate entries ran: nothing went through the relaxed EMD's borrower
        assert _ops.remd_borrow_stats == before
    check_against_float64(lb, eng)


# ------------------------------------------------------------------ 2. the remd cases without the grouped entry
@pytest.mark.parametrize("lb", REMD_MAP_TEMPORAL)
def test_remd_cases_without_the_grouped_entry_borrow_after_the_weighted_entry(lb, monkeypatch):
    """STROTSS_GROUPED_LOSSES=0: the separate weighted content entry, then the relaxed EMD borrowing from its workspace --
    the borrow is taken once per (region, style), the step stays within 1e-5 of the grouped one and within the bounds of
    float64"""
    from nn import _ops
    idx = _indices(lb)
    eng = _engine(lb)
    eng.forward_backward(idx)
    torch.cuda.synchronize()
    monkeypatch.setenv("STROTSS_GROUPED_LOSSES", "0")
    assert not _ops.step_losses_available()
    eng2 = _engine(lb)
    before = dict(_ops.remd_borrow_stats)
    eng2.forward_backward(idx)
    torch.cuda.synchronize()
    calls = sum(len(s) if C.blend_of(C.ROWS[lb]) else 1 for s in C.problem(lb)["s_idx"])
    if eng2._styles[0][0][0].panels is not None:       # x3 panels exist: the borrow is what ran
        assert _ops.remd_borrow_stats["borrowed"] == before["borrowed"] + calls
        assert _ops.remd_borrow_stats["plain"] == before["plain"]
    la, lb_ = eng.losses(), eng2.losses()
    for key in ("loss", "loss_c", "loss_s", "loss_t"):
        assert abs(la[key] - lb_[key]) <= 1e-5 * max(1.0, abs(la[key])), (key, la[key], lb_[key])
    for ga, gb in zip(eng.gp, eng2.gp):
        assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())
    check_against_float64(lb, eng2, what="ungrouped")


# ------------------------------------------------------------------ 3. three forms of the step give the same bits
def _state(eng):
    return [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()] + \
        [t.loss.clone() for t in eng._pixel_terms]                # the temporal term's scalars, where there is one


@pytest.mark.parametrize("lb", BORROWING)
def test_eager_graph_and_device_draw_give_the_same_bits(lb, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    from nn import rand
    from nn import strotss_utils as SU
    row, P = C.ROWS[lb], C.problem(lb)
    (h, w), n, steps = row[4], P["n_samples"], 3
    cmasks = [None] if C.masks_of(row) is None else [cm for cm, _ in C.masks_of(row)]
    rng = np.random.default_rng(5)
    idx = [_indices(lb)] + [[torch.from_numpy(O.make_indices(h, w, True, n, rng, mask=cm)).to(DEV) for cm in cmasks]
                            for _ in range(steps - 1)]
    # eager with injected indices against the captured graph replayed
    finals = []
    for graph in (False, True):
        eng = _engine(lb, deterministic=True)
        if graph:
            eng.capture_graph(idx[0])
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")    # a device-to-host read inside a replayed step raises
        try:
            for i in idx:
                eng.step(i)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        if row[0] == "sliced":
            assert int(eng._sliced_counter.item()) == steps * {"one": 1, "blend": 2, "regions": 2}[row[1]]
        finals.append((_state(eng), eng.losses()))
    assert finals[0][1] == finals[1][1]
    for a, b in zip(finals[0][0], finals[1][0]):
        assert torch.equal(a, b), "eager vs graph replay"
    # the device draw (captured) against a second engine that is given the host twin's draws
    masks = [None if cm is None else cm[:, :, 0].astype(bool) for cm in cmasks]
    dev_eng, host = _engine(lb, deterministic=True), _engine(lb, deterministic=True)
    if not dev_eng.enable_device_draw(17, 0, masks):
        assert row[1] == "regions"             # a region with fewer candidates than samples: the engine declines
        return
    dev_eng.capture_graph()
    stream = rand.PhiloxStream(17, 0)
    for _ in range(steps):
        dev_eng.step()
        host.step([torch.from_numpy(SU.make_indices_np(h, w, True, n, stream, m)).to(DEV) for m in masks])
    torch.cuda.synchronize()
    assert dev_eng.losses() == host.losses()
    for a, b in zip(_state(dev_eng), _state(host)):
        assert torch.equal(a, b), "device draw vs host twin"


# ------------------------------------------------------------------ 4. without x3 panels
def test_borrowing_cases_without_x3_panels_in_a_child_process():
    """STROTSS_X3=0 is read once per process: both borrowers pass NULL panels and still take the norms from the weighted
    entry's workspace.  A fresh child compares the sinkhorn and sliced cases with a weight map to the same bounds."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "x3_off"], env=dict(os.environ, STROTSS_X3="0"),
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-8000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] == BORROWING and res["panels"] is False


def _child():
    import ctypes as ct
    from nn import _hip, _ops
    for lb in BORROWING:
        eng = _engine(lb)
        eng.forward_backward(_indices(lb))
        torch.cuda.synchronize()
        check_against_float64(lb, eng, what="x3_off")
    # what the library hands out in this process: no panels
    pf = eng.pf[0]
    n = len(C.problem(BORROWING[-1])["idx"][0])
    nb = _hip.lib().strotss_selfsim_workspace_bytes(n, pf.shape[1])
    ws = _ops.workspaces.get("selfsim", nb, pf.device)
    rp, xp = ct.c_void_p(), ct.c_void_p()
    _hip.check(_hip.lib().strotss_selfsim_pred_panels(_hip.ptr(ws), nb, n, pf.shape[1], ct.byref(rp), ct.byref(xp)), "panels")
    print(json.dumps({"cases": BORROWING, "panels": bool(xp.value)}))


# ------------------------------------------------------------------ 5. the restatement against the _engine_case oracles
def _problem_of_engine_case(h, w, n, cw, n_targets, ramp):
    """the inputs _engine_case of the weight-map and temporal tests makes (regions = 1, seed 0), as a _step_ref problem"""
    from nn.model import synthetic_weights
    import test_hip_content_weight as TCW
    import test_hip_temporal as TT
    import test_hip_temporal_long as TTL
    content, style = TT._img(h, w, 1), TT._img(56, 60, 2)
    rng = np.random.default_rng(0)
    s_idx = O.make_indices(56, 60, False, n, rng)
    idx = O.make_indices(h, w, True, n, rng)
    wmap = None
    if cw:
        wmap = TCW.ramp_map(h, w) if ramp else torch.from_numpy(np.tile(np.linspace(0.0, 1.2, w, dtype=np.float32), (h, 1)))
    if n_targets == 1:
        temporal = [TT._temporal_inputs(h, w) + (40.0,)]
    else:
        temporal = [(tg, c, lam) for (tg, c), lam in zip(TTL._long_targets(h, w, n_targets), TTL.LAMS)] if n_targets else []
    return dict(weights=synthetic_weights('16', 0), content=content, styles=[style], s_idx=[[s_idx]], idx=[idx], alpha=8.0,
                denom=2.0 + 8.0 + 1.0 / 8.0, h=h, w=w, n_samples=n, wmap=wmap, temporal=temporal)


def test_restatement_equals_the_weight_map_and_temporal_oracles_themselves():
    """tests/test_step_cases_cpu.py compares the restatement with a transcription of these oracles (they build an engine first
    and cannot run without a GPU); here with the functions themselves, at 1e-12"""
    import test_hip_content_weight as TCW
    import test_hip_temporal as TT
    import test_hip_temporal_long as TTL
    h = w = 64
    n = 256

    def close(a, b):
        assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b)), (float(a), float(b))

    def grads_close(got, grads):
        assert len(grads) == 6
        for a, b in zip(got["grads"], grads):
            assert float((a - b).norm()) <= 1e-12 * float(b.norm())
    _, _, loss, lc, grads = TCW._engine_case(h, w, n=n)
    got = R.reference_step(_problem_of_engine_case(h, w, n, True, 0, True), ("remd",))
    close(got["loss"], loss), close(got["loss_c"], lc), grads_close(got, grads)
    _, _, ref = TT._engine_case(h, w, n=n, cw=True)
    got = R.reference_step(_problem_of_engine_case(h, w, n, True, 1, False), ("remd",))
    close(got["loss"], ref["loss"]), close(got["loss_c"], ref["loss_c"]), close(got["loss_t"], ref["loss_t"])
    grads_close(got, ref["grads"])
    _, _, ref = TTL._engine_case(h, w, n=n, cw=True)
    got = R.reference_step(_problem_of_engine_case(h, w, n, True, 3, False), ("remd",))
    close(got["loss"], ref["loss"]), close(got["loss_c"], ref["loss_c"]), close(got["loss_t"], ref["loss_t"])
    for a, b in zip(got["loss_t_terms"], ref["terms"]):
        close(a, b)
    grads_close(got, ref["grads"])


# ------------------------------------------------------------------ 6. the command line
@pytest.mark.parametrize("transport", ["sliced", "sinkhorn"])
def test_cli_video_with_transport_weight_map_and_temporal_frames(transport, tmp_path, monkeypatch):
    """three frames, --temporal_frames 1 2 3 (frame 2 has one earlier frame, frame 3 two; offset 3 never applies), a weight
    map and the transport at once: the settings of test_hip_sliced.test_cli_sliced_video"""
    import run_strotss
    from PIL import Image
    from test_hip_color import _moved_frames, _texture
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    cmap = np.tile(np.linspace(0, 255, 64).astype(np.uint8), (48, 1))
    cmap[16:22] = 0
    Image.fromarray(cmap).save(tmp_path / "map.png")
    extra = {"sliced": ["--style_transport", "sliced", "--sliced_projections", "32"],
             "sinkhorn": ["--style_transport", "sinkhorn", "--sinkhorn_iters", "10"]}[transport]
    key = R.TRANSPORT_KEY[transport]
    stems = [os.path.splitext(os.path.basename(q))[0] for q in paths]
    outs = []
    for tag in ("a", "b"):
        trace = []
        run_strotss.run(run_strotss.build_parser().parse_args(
            [frames, style, "--video", "--compute_flow", "-o", str(tmp_path / tag), "--max_size", "64", "--level", "1",
             "--max_iter", "10", "--temporal_frames", "1", "2", "3", "--content_weight_map", str(tmp_path / "map.png")] + extra),
            trace=trace)
        assert len(stems) == 3 and sorted(os.listdir(tmp_path / tag)) == sorted(t + ".jpg" for t in stems)
        outs.append([open(tmp_path / tag / (t + ".jpg"), "rb").read() for t in stems])
        assert len(trace) == 3
        for t, rec in enumerate(trace, start=1):
            steps = [s for scale in rec for s in scale["steps"]]
            assert steps and all(key in s and np.isfinite(s[key]) and s[key] > 0 for s in steps)
            assert all(("loss_t" in s) == (t > 1) for s in steps)
            if t == 3:
                assert all(len(s["loss_t_terms"]) == 2 for s in steps)
    assert outs[0] == outs[1], "two runs under STROTSS_DETERMINISTIC=1 differ"


if __name__ == "__main__":
    assert sys.argv[1:] == ["x3_off"]
    _child()
