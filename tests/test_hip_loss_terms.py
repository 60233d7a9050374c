"""Every loss entry of the C ABI (but the Sinkhorn entries and strotss_rows_gemm_bwd: tests/test_hip_sinkhorn.py), one term at a time, at every case of tests/_loss_cases.py (the step's shape, ragged sample
counts, the tie-list limit ns = 2048, n = 1 / 2 / 37, flat regions, d = 3100) against the float64 restatement of
tests/_loss_ref.py: every scalar within TOL_SCALAR relative, every gradient within TOL_GRAD of max|ref| (the L1 terms
outside the flip-aware bound).  The grouped entries are called once per term with only that term's g non-zero.  Every call:
the gradient buffer holds a seeded base (the entries ADD) and a sentinel in its padding rows and columns (left unchanged),
and the cached workspaces are filled with NaN bytes first (a read of workspace memory the call did not write shows).
The measured worst values are in DESIGN.md section 6."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _loss_cases as LC
import _loss_ref as LR
from _loss_harness import DEV, LC_pad, check_gradient, check_scalar, fbuf, report, run_entry

pytestmark = pytest.mark.gpu

CASES = [c[0] for c in LC.CASES if c[4] != "public"]
PUBLIC = [c for c in LC.LABELS if c not in CASES]


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@pytest.fixture(scope="module", params=CASES, ids=[f"case_{c}" for c in CASES])
def R(request):
    return refs_of(request.param)


class Refs:
    """float64 references of one case, each computed once"""

    def __init__(self, label):
        self.c = LC.make_case(label)
        self._memo = {}

    def get(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    @property
    def col_weight(self):
        w = np.random.default_rng(5).random(self.c.n) * 2.0
        w[::7] = 0.0
        return w

    def selfsim(self, weighted=False):
        c = self.c
        return self.get(("ss", weighted), lambda: LR.selfsim(c.y, c.c, self.col_weight if weighted else None))

    def moment(self):
        return self.get("mom", lambda: LR.moment(self.c.x, self.c.y))

    def remd(self, metric):
        c = self.c
        return self.get(("remd", metric), lambda: LR.remd(c.x, c.y, c.gx, c.gy, metric))

    def palette(self, yuv):
        c = self.c
        return self.get(("pal", yuv), lambda: LR.palette(c.x, c.y, c.gx, c.gy, yuv))


_refs = {}


def refs_of(label):
    if label not in _refs:
        _refs.clear()                       # one case's references at a time (tests are grouped by case)
        _refs[label] = Refs(label)
    return _refs[label]


def check_dups(what, case, g0):
    for grp in case.dup_groups_y:
        for k in grp[1:]:
            assert np.array_equal(g0[k], g0[grp[0]]), (what, "duplicate prediction rows differ", int(k))


# ------------------------------------------------------------------ the cost / covariance error the tolerance model states
def test_separate_cost_and_moment_stats_error(ops, R):
    """the prediction rows' cosine self-distances on the bf16x3 / f32 cost core within LR.EPS_COST of float64, and the
    style side's mean and covariance (strotss_moment_stats) within LR.cov_tau: the errors the flip-aware bounds assume"""
    c = R.c
    label = c.label
    by, bx = fbuf(c.y), fbuf(c.x)
    if os.environ.get("STROTSS_X3") == "0":
        ry = ops.row_inv_norm(by, c.n)
        D = ops.cosine_distance(by, ry, c.n, by, ry, c.n)
    else:
        ry, py = ops.row_inv_norm_x3(by, c.n)
        D = ops.cosine_distance_x3(py, ry, c.n, py, ry, c.n, by.shape[1])
    D = D[:, :c.n].double().cpu().numpy()
    err = np.abs(D - LR.cos_dist(c.y, c.y)).max()
    report("cost_err", label, f"{err:.3e}")
    bx = fbuf(c.x)
    mean, cov = ops.moment_stats(bx, c.ns, c.d)
    m64, S64 = LR.moment_stats(c.x)
    tc, tm = LR.cov_tau(c.x)
    ec = np.abs(cov[:c.d, :c.d].double().cpu().numpy() - S64)
    em = np.abs(mean[:c.d].double().cpu().numpy() - m64)
    report("cov_err_over_tau", label, f"{(ec / tc).max():.3e} mean {(em / tm).max():.3e}")
    assert err <= LR.EPS_COST
    assert (ec <= tc).all() and (em <= tm).all()


# ------------------------------------------------------------------ the separate entries
@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_separate_selfsim(ops, R, weighted):
    c = R.c
    label = c.label
    l, g, b, namb = R.selfsim(weighted)
    report(f"ambiguous:selfsim{'_w' if weighted else ''}", label, f"{namb} of {c.n * c.n}")
    by, bc = fbuf(c.y), fbuf(c.c)
    gs = 0.75
    if weighted:
        w = torch.zeros(LC_pad(c.n), dtype=torch.float32, device=DEV)
        w[:c.n] = torch.as_tensor(R.col_weight, dtype=torch.float32, device=DEV)
        fn = lambda gp, lo: ops.selfsim_weighted_fwd_bwd(by, bc, w, c.n, c.d, gs, gp, lo[0])
    else:
        fn = lambda gp, lo: ops.selfsim_fwd_bwd(by, bc, c.n, c.d, gs, gp, lo[0])
    got, loss, _ = run_entry(ops, fn, c.n, c.d, np.abs(g).max() * gs, 1)
    check_scalar("selfsim", label, loss[0, 0], l)
    check_gradient("selfsim_w" if weighted else "selfsim", label, got / gs, g, b)


def test_separate_moment(ops, R):
    c = R.c
    label = c.label
    l, g, b, namb = R.moment()
    report("ambiguous:moment", label, f"{namb} of {c.d * c.d + c.d}")
    bx, by = fbuf(c.x), fbuf(c.y)
    mean, cov = ops.moment_stats(bx, c.ns, c.d)
    gs = 1.5
    got, loss, g0 = run_entry(ops, lambda gp, lo: ops.moment_fwd_bwd(mean, cov, by, c.n, c.d, gs, gp, lo[0]), c.n, c.d,
                              np.abs(g).max() * gs, 2)
    check_scalar("moment", label, loss[0, 0], l)
    check_gradient("moment", label, got / gs, g, b)
    check_dups("moment", c, g0)


@pytest.mark.parametrize("form", ["plain", "swapped", "after_selfsim"])
def test_separate_remd_cos(ops, R, form):
    c = R.c
    label = c.label
    l, g, row, _ = R.remd("cos")
    report("branch:remd_cos", label, "row" if row else "col")
    bx, by, bc = fbuf(c.x), fbuf(c.y), fbuf(c.c)
    rs, panels = ops.row_inv_norm_x3(bx, c.ns)
    rs = ops.row_inv_norm(bx, c.ns)
    gs = 2.0

    def fn(gp, lo):
        if form == "after_selfsim":
            ops.selfsim_fwd_bwd(by, bc, c.n, c.d, 1.0, torch.zeros_like(gp), lo[1])
            ops.remd_cos_fwd_bwd_after_selfsim(bx, rs, panels, c.ns, by, c.n, c.d, gs, gp, lo[0])
        else:
            ops.remd_cos_fwd_bwd(bx, rs, c.ns, by, c.n, c.d, gs, gp, lo[0], swapped=form == "swapped")
    got, loss, g0 = run_entry(ops, fn, c.n, c.d, np.abs(g).max() * gs, 3)
    check_scalar("remd_cos", label, loss[0, 0], l)
    check_gradient("remd_cos", label, got / gs, g)
    check_dups("remd_cos", c, g0)


@pytest.mark.parametrize("yuv", [True, False], ids=["yuv", "rgb"])
@pytest.mark.parametrize("swapped", [False, True], ids=["plain", "swapped"])
def test_separate_palette(ops, R, yuv, swapped):
    c = R.c
    label = c.label
    l, g, row, b = R.palette(yuv)
    report(f"branch:palette_{'yuv' if yuv else 'rgb'}", label, "row" if row else "col")
    bx, by = fbuf(c.x), fbuf(c.y)
    gs = 0.5
    got, loss, g0 = run_entry(ops, lambda gp, lo: ops.palette_remd_fwd_bwd(bx, c.ns, by, c.n, gs, gp, lo[0], rgb_to_yuv=yuv,
                                                                            swapped=swapped),
                              c.n, c.d, np.abs(g).max() * gs, 4)
    check_scalar("palette", label, loss[0, 0], l)
    assert np.all(got[:, 3:] == 0.0)
    check_gradient("palette", label, got[:, :3] / gs, g, b)
    check_dups("palette", c, g0)


@pytest.mark.parametrize("metric", ["l2", "both"])
def test_separate_remd_metric(ops, R, metric):
    c = R.c
    label = c.label
    l, g, row, b = R.remd(metric)
    report(f"branch:remd_{metric}", label, "row" if row else "col")
    bx, by = fbuf(c.x), fbuf(c.y)
    gs = 1.25
    got, loss, g0 = run_entry(ops, lambda gp, lo: ops.remd_metric_fwd_bwd(bx, c.ns, by, c.n, c.d, metric, gs, gp, lo[0]),
                              c.n, c.d, np.abs(g).max() * gs, 5)
    check_scalar(f"remd_{metric}", label, loss[0, 0], l)
    check_gradient(f"remd_{metric}", label, got / gs, g, b)
    check_dups(f"remd_{metric}", c, g0)


# ------------------------------------------------------------------ the grouped entries, one term at a time
TERMS = ("content", "moment", "remd", "palette")
G_TERM = (0.7, 0.3, 0.9, 0.4)


def _term_ref(R, term, weighted=False):
    if term == "content":
        l, g, b, _ = R.selfsim(weighted)
        return l, g, b
    if term == "moment":
        l, g, b, _ = R.moment()
        return l, g, b
    if term == "remd":
        l, g, _, _ = R.remd("cos")
        return l, g, None
    l, g, _, b = R.palette(True)
    full, fb = np.zeros_like(R.c.y), np.zeros_like(R.c.y)
    full[:, :3], fb[:, :3] = g, b
    return l, full, fb


def _target(ops, x, ns, d):
    from nn.engine import StyleTarget
    return StyleTarget.build(fbuf(x), ns, d)


@pytest.mark.parametrize("entry", ["step", "cw_none", "cw_weighted"])
def test_grouped_one_style(ops, R, entry):
    """step_losses_fwd_bwd and step_losses_cw_fwd_bwd with one style (with and without column weights), once per term"""
    assert ops.step_losses_available()
    c = R.c
    label = c.label
    by, bc = fbuf(c.y), fbuf(c.c)
    t = _target(ops, c.x, c.ns, c.d)
    weighted = entry == "cw_weighted"
    cw = None
    if weighted:
        cw = torch.zeros(LC_pad(c.n), dtype=torch.float32, device=DEV)
        cw[:c.n] = torch.as_tensor(R.col_weight, dtype=torch.float32, device=DEV)
    refs = [_term_ref(R, term, weighted and term == "content") for term in TERMS]
    for k, term in enumerate(TERMS):
        gv = [0.0] * 4
        gv[k] = G_TERM[k]

        def fn(gp, lo):
            if entry == "step":
                ops.step_losses_fwd_bwd(by, bc, c.n, c.d, t.feats, t.inv_norm, t.panels, t.ns, t.mean, t.cov, *gv, gp,
                                        lo[0], lo[1], lo[2], lo[3])
            else:
                s = ops.make_style_set([t], [1.0])
                ops.step_losses_cw_fwd_bwd(by, bc, c.n, c.d, cw, s, *gv, gp, lo[0], lo[1], lo[2], lo[3])
        ref_l, ref_g, ref_b = refs[k]
        got, loss, g0 = run_entry(ops, fn, c.n, c.d, np.abs(ref_g).max() * G_TERM[k], 10 + k)
        for kk in range(4):
            check_scalar(f"{entry}:{TERMS[kk]}", label, loss[kk, 0], refs[kk][0])
        check_gradient(f"{entry}:{term}", label, got / G_TERM[k], ref_g, ref_b)
        if term != "content":
            check_dups(f"{entry}:{term}", c, g0)


@pytest.mark.parametrize("k", [1, 2, 3, 4])
@pytest.mark.parametrize("entry", ["blend", "cw_none", "cw_weighted"])
def test_grouped_blend(ops, k, entry):
    """step_losses_blend_fwd_bwd / step_losses_cw_fwd_bwd with K = 1..4 styles of their own weights (ns 1024, 777, 2048,
    1500, the last with a duplicate group) against the "step" case's prediction rows: per term, sum_k w_k dL_k"""
    assert ops.step_losses_available()
    R = refs_of("step")
    c = R.c
    styles = LC.blend_styles(k)
    weights = LC.BLEND_WEIGHTS[:k]
    by, bc = fbuf(c.y), fbuf(c.c)
    targets = [_target(ops, x, x.shape[0], c.d) for x, _ in styles]
    weighted = entry == "cw_weighted"
    cw = None
    if weighted:
        cw = torch.zeros(LC_pad(c.n), dtype=torch.float32, device=DEV)
        cw[:c.n] = torch.as_tensor(R.col_weight, dtype=torch.float32, device=DEV)
    per_style = []
    for (x, gx) in styles:
        lm, gm, bm, _ = LR.moment(x, c.y)
        lr, gr, _, _ = LR.remd(x, c.y, gx, c.gy, "cos")
        lp, gp3, _, bp3 = LR.palette(x, c.y, gx, c.gy, True)
        gp, bp = np.zeros_like(gr), np.zeros_like(gr)
        gp[:, :3], bp[:, :3] = gp3, bp3
        per_style.append(((lm, gm, bm), (lr, gr, None), (lp, gp, bp)))
    lc, gc, bc_, _ = R.selfsim(weighted)
    s = ops.make_style_set(targets, list(weights))
    for t_i, term in enumerate(TERMS):
        gv = [0.0] * 4
        gv[t_i] = G_TERM[t_i]
        if term == "content":
            ref_g, ref_b = gc, bc_
        else:
            parts = [ps[t_i - 1] for ps in per_style]
            ref_g = sum(w * p[1] for w, p in zip(weights, parts))
            ref_b = None if parts[0][2] is None else sum(w * p[2] for w, p in zip(weights, parts))

        def fn(gp, lo):
            if entry == "blend":
                ops.step_losses_blend_fwd_bwd(by, bc, c.n, c.d, s, *gv, gp, lo[0], lo[1], lo[2], lo[3])
            else:
                ops.step_losses_cw_fwd_bwd(by, bc, c.n, c.d, cw, s, *gv, gp, lo[0], lo[1], lo[2], lo[3])
        got, loss, _ = run_entry(ops, fn, c.n, c.d, np.abs(ref_g).max() * G_TERM[t_i], 20 + t_i)
        check_scalar(f"{entry}{k}:content", "step", loss[0, 0], lc)
        for si in range(k):
            for kk in range(3):
                check_scalar(f"{entry}{k}:{TERMS[kk + 1]}[{si}]", "step", loss[kk + 1, si], per_style[si][kk][0])
        check_gradient(f"{entry}{k}:{term}", "step", got / G_TERM[t_i], ref_g, ref_b)


# ------------------------------------------------------------------ the public entries at d = 3100 (second column trip)
@pytest.mark.parametrize("label", PUBLIC)
@pytest.mark.parametrize("term", ["self_similarity", "moment_matching", "cosine", "l2", "both"])
def test_public_entries(label, term):
    from nn import losses
    R = refs_of(label)
    c = R.c
    x = torch.as_tensor(c.x, dtype=torch.float32, device=DEV)
    y = torch.as_tensor(c.y, dtype=torch.float32, device=DEV).requires_grad_(True)
    cc = torch.as_tensor(c.c, dtype=torch.float32, device=DEV)
    if term == "self_similarity":
        l, g, b, _ = R.selfsim()
        out = losses.self_similarity(y, cc)
    elif term == "moment_matching":
        l, g, b, _ = R.moment()
        out = losses.moment_matching(x, y)
    else:
        l, g, _, b = R.remd("cos" if term == "cosine" else term)
        out = losses.relaxed_emd(x, y, term)
    got, = torch.autograd.grad(out, y)
    torch.cuda.synchronize()
    check_scalar(term, label, float(out), l)
    check_gradient(term, label, got.double().cpu().numpy(), g, b)


# ------------------------------------------------------------------ the f32 cost / covariance GEMMs
def test_separate_entries_on_the_f32_path():
    """STROTSS_X3=0 (read once per process: a child process) keeps the cost and covariance products on the f32 MFMA: the
    separate entries at the step's shape and at ragged sample counts must pass the same checks"""
    if os.environ.get("STROTSS_X3") == "0":
        pytest.skip("already inside the forced run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, STROTSS_X3="0")
    out = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu", "-s",
                          "-k", "separate and not f32_path and (case_step or case_ragged_n1000_ns777)"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=900)
    print("\n".join(line.replace("MEASURE ", "MEASURE f32:") for line in out.stdout.splitlines() if "MEASURE" in line))
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert " passed" in out.stdout and " skipped" not in out.stdout
