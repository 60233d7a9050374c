"""GPU: every entry stays inside the scratch bytes its `strotss_*_workspace_bytes` twin declares, and needs nothing of
their previous content ("The scratch contract").  Each case calls the product's own wrapper with a
tests/_scratch_guard.py GuardedWorkspaces -- every workspace an exact-size view between two pattern-filled guard bands, the
interior holding the same quiet NaN -- and with every output in a guarded tensor of its own, and then asks:
  a/b. inputs from the family's existing case module, the call through nn._ops;
  c.   every guard of every workspace and output still holds the pattern, bit for bit;
  d.   no output element inside the declared extent still holds the fill; padding the entry leaves alone still does;
  e.   the result meets the float64 reference of the family's existing test at that test's bound (imported, not copied):
       a read of scratch the call did not write is a NaN here.
Step d does not apply to an output the entry ADDS into (gpred, gimg): it holds a base before the call, and what the entry
wrote shows in the value comparison alone.  Not guarded: what a wrapper allocates itself and offers no argument for
(moment_stats' mean and cov), and the outputs of the helpers that only prepare inputs (winograd_weights, row_inv_norm_x3,
pool_mean).  Then poison() and a second call: the same bits.  Nothing here runs an under-sized request on purpose; that the guards
bite is shown on the CPU by tests/test_scratch_guard_cpu.py.

Convolution: one ragged case per (route, direction) of _route_cases.DEFAULT_CASES plus the odd-tile-count shapes of the three
F(4x4,3x3) GEMM routes (T = 2795, 289, 187), F4_fused_f32 (no workspace, guarded outputs), the forward plain and with its pool /
sign-word epilogue, the data-gradient plain, masked and accumulating, and conv3x3_dgrad_unpool on a split-K layer in front of
an odd-sized (27 x 35) map.  Losses: the entries that take ws= at the smallest ragged case of their case module and, for
the entries of _loss_cases, at the step's n = ns = 1024 (selfsim, selfsim_weighted, remd plain and with borrowed panels,
moment_stats, moment_fwd_bwd, step_losses, step_losses_blend, step_losses_cw, palette_remd, remd_metric, sinkhorn plain, metric,
step and log).  sliced and palette_sliced at their smallest case with both counts off the 64-row tile and at n = ns = 1024 (the
Sinkhorn case modules have no n = 1024 case with a float64 reference: that count is the engine's).  The pixel side:
tv_fwd_bwd, detail_fwd_bwd, temporal_fwd_bwd, temporal_multi_fwd_bwd (four targets), guided_smooth, guided_upsample (both
modes), optical_flow, color_stats, detail_map and scribble_labels at their case module's smallest size and at one with both
sides odd.  The engine: a 64 px deterministic StepEngine whose Workspaces is the guarded class, eager, captured and
replayed, bit for bit the run on the product's class; and a 42 x 64 one with all four pixel-space terms, whose zeroed
workspaces are the engine's and of exactly the library's sizes.

Each run appends (entry, shape, tag, declared bytes, high-water mark) to profiles/scratch_contracts.txt when the whole file
ran; nothing is asserted on it."""
import os
import zlib

import numpy as np
import pytest
import torch

import _loss_cases as LC
import _route_cases as RC
import _scratch_guard as SG
import _transport_ref as TR
from _loss_harness import DEV, LC_pad, check_gradient, check_scalar, fbuf, gpred_base

pytestmark = pytest.mark.gpu

NAN = float("nan")
F32 = torch.float32
RECORD = {}                              # family -> lines
FAMILIES = ("conv", "loss", "pixel", "engine")


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@pytest.fixture
def ws(ops, monkeypatch):
    """a fresh GuardedWorkspaces that also stands where the module-level instance stood: a helper of another test module
    that passes no ws= draws from it as well"""
    g = SG.GuardedWorkspaces()
    monkeypatch.setattr(ops, "workspaces", g)
    return g


@pytest.fixture(scope="module", autouse=True)
def _record_file():
    yield
    if set(RECORD) != set(FAMILIES):
        return                           # a partial run: the committed record stays
    try:
        with open(os.path.join(RC.ROOT, "profiles", "scratch_contracts.txt"), "w") as f:
            f.write("# tests/test_hip_scratch_contracts.py: entry | shape | workspace tag[bytes asked] | declared bytes | "
                    "high-water mark (offset of the last byte written, -1: untouched)\n")
            for fam in FAMILIES:
                f.write("".join(line + "\n" for line in RECORD[fam]))
    except OSError:
        pass


@pytest.fixture(autouse=True)
def _stop_after_a_gpu_error():
    """a HIP error is sticky: nothing more of this file is started on a device that has reported one"""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"the device reported an error, the remaining scratch-contract cases are not run: {e}", returncode=3)


def record(family, entry, shape, marks):
    for tag, (nbytes, high) in sorted(marks.items()):
        RECORD.setdefault(family, []).append(f"{entry} | {shape} | {tag} | {nbytes} | {high}")


def checked(ws, *guards):
    torch.cuda.synchronize()
    for g in guards:
        g.check()
    return ws.check()


# ------------------------------------------------------------------ convolution
def _pick(route, direction):
    """the smallest case of DEFAULT_CASES on (route, direction) with a partial 4 x 4 tile"""
    c = [c for c in RC.DEFAULT_CASES if c[0] == route and c[1] == direction and (c[2] % 4 or c[3] % 4)]
    return min(c, key=lambda c: c[2] * c[3] * c[4] * c[5])


ODD_T = [c for c in RC.DEFAULT_CASES if c[0] in ("F4_gemm_f32", "F4_x3_gemm_128", "F4_x3_gemm_64")
         and (-(-c[2] // 4) * -(-c[3] // 4)) % 2]
CONV_CASES = [_pick(r, d) for r in RC.ROUTES for d in ("fwd", "dgrad") if (r, d) != ("direct", "fwd")]
CONV_CASES += [c for c in ODD_T if c not in CONV_CASES]


def test_conv_cases_reach_every_route_and_an_odd_tile_count():
    """(no default route sends a forward to the one-pass direct kernel: tests/test_route_cases_cpu.py)"""
    have = {(c[0], c[1]) for c in CONV_CASES}
    assert have == {(r, d) for r in RC.ROUTES for d in ("fwd", "dgrad")} - {("direct", "fwd")}
    for r in ("F4_gemm_f32", "F4_x3_gemm_128", "F4_x3_gemm_64"):
        for d in ("fwd", "dgrad"):
            assert any(c[0] == r and c[1] == d for c in ODD_T), (r, d)


@pytest.mark.parametrize("case", CONV_CASES, ids=RC.case_id)
def test_conv_route_inside_its_workspace(ops, ws, case):
    import test_hip_conv_routes as CR
    from nn import _hip
    route, direction, h, w, cin, cout = case
    M = RC._model()
    assert M.conv_route(h, w, cin, cout, dgrad=direction == "dgrad") == route
    tol = CR.TOL.get(route, 5e-5)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(RC.case_id(case).encode()))
    x = torch.relu(torch.randn(1, h, w, cin, generator=g, device="cuda"))
    wt = torch.randn(3, 3, cin, cout, generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g, device="cuda") * 0.1
    tile = M.winograd_tile(h, w, cin, cout) if M.use_winograd(cin, cout) else 0
    shape = f"{h}x{w}x{cin}to{cout}"

    def within(what, got, ref):
        mx, _ = CR._err(got, ref)
        print(f"{RC.case_id(case):42s} {what:13s} max {mx:.2e} (tol {tol:.0e})")
        assert mx < tol, (RC.case_id(case), what, mx, tol)          # (a NaN fails it)

    if direction == "fwd":
        if tile:
            u = ops.winograd_weights(wt.permute(3, 2, 0, 1), tile)
            fwd = lambda **kw: ops.conv3x3_winograd_fwd(x, u, b, ws=ws, **kw)
        else:
            w_tok = wt.permute(0, 1, 3, 2).reshape(9, cout, cin).contiguous()
            fwd = lambda **kw: ops.conv3x3_relu_fwd(x, w_tok, b, ws=ws, **kw)
        ref = torch.relu(CR._conv64(x, wt) + b.double())
        out, go = SG.guarded((1, h, w, cout), F32, NAN, name="out")
        fwd(out=out)
        marks = checked(ws, go)
        assert go.untouched() == 0
        within("fwd", out, ref)
        record("conv", f"{route}-fwd", shape, marks)
        # the trunk's call: everything the epilogue writes at once, from dirty scratch
        ws.poison()
        out2, go2 = SG.guarded((1, h, w, cout), F32, NAN, name="out")
        extra, guards = {}, [go2]
        extra["pool_out"], gp = SG.guarded((1, h // 2, w // 2, cout), F32, NAN, name="pool_out")
        extra["pool_code"], gc = SG.guarded((1, h // 2, w // 2, cout), torch.uint8, 9, name="pool_code")
        guards += [gp, gc]
        if route.startswith("F4"):
            nb = int(_hip.lib().strotss_relu_bits_bytes(h, w, cout))
            tiles = -(-h // 4) * -(-w // 4)
            assert nb == tiles * cout * 4
            extra["relu_bits_out"], gb = SG.guarded((nb // 4 // cout, cout), torch.int32, SG.PATTERN, name="relu_bits_out")
            guards.append(gb)
        fwd(out=out2, **extra)
        marks = checked(ws, *guards)
        assert all(gd.untouched() == 0 for gd in guards)
        assert torch.equal(out2, out), "the second call, with the epilogue outputs, changes the activation"
        want = torch.nn.functional.max_pool2d(out.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
        assert torch.equal(extra["pool_out"], want), "pooled copy"
        code = torch.empty((1, h // 2, w // 2, cout), dtype=torch.uint8, device="cuda")
        ops.maxpool2_fwd(out, code=code)
        assert torch.equal(extra["pool_code"], code), "argmax codes"
        if "relu_bits_out" in extra:
            words, valid = CR._sign_words(out)
            bits = extra["relu_bits_out"].long() & 0xFFFFFFFF
            assert torch.equal(bits & valid, words)
        record("conv", f"{route}-fwd+epilogue", shape, marks)
        return

    gy = torch.randn(1, h, w, cout, generator=g, device="cuda")
    if tile:
        u = ops.winograd_weights(wt.flip(0, 1).permute(2, 3, 0, 1), tile)
        dg = lambda **kw: ops.conv3x3_winograd_dgrad(gy, u, cin, ws=ws, **kw)
        can_add = route != "F2_gemm_f32"                   # (F(2x2,3x3) overwrites; the library refuses accumulate there)
    else:
        w_tik = wt.flip(0, 1).reshape(9, cin, cout).contiguous()
        dg = lambda **kw: ops.conv3x3_dgrad(gy, w_tik, cin, ws=ws, **kw)
        can_add = ops.conv3x3_dgrad_accumulates(h, w, cout, cin)
    ref = CR._conv64(gy, wt.flip(0, 1).transpose(2, 3))
    ref_masked = ref * (x > 0)

    def call(what, want, **kw):
        out, go = SG.guarded((1, h, w, cin), F32, NAN, name="gin")
        dg(out=out, **kw)
        marks = checked(ws, go)
        assert go.untouched() == 0
        within(what, out, want)
        return out, marks
    plain, marks = call("dgrad", ref)
    record("conv", f"{route}-dgrad", shape, marks)
    ws.poison()
    again, _ = call("dgrad again", ref)
    assert torch.equal(again, plain), "the second call from dirty scratch gives other bits"
    ws.poison()
    masked, _ = call("dgrad_masked", ref_masked, act_in=x)
    mask_kw = {"act_in": x}
    if route.startswith("F4"):
        mask_kw["relu_bits"] = CR._sign_words(x)[0].int()
        ws.poison()
        by_bits, _ = call("dgrad_bits", ref_masked, relu_bits=mask_kw["relu_bits"])
        assert torch.equal(by_bits, masked)
    if can_add:
        ws.poison()
        pre = torch.randn(1, h, w, cin, generator=g, device="cuda")
        acc, ga = SG.guarded((1, h, w, cin), F32, NAN, name="gin")
        acc.copy_(pre)
        dg(out=acc, accumulate=True, **mask_kw)
        marks = checked(ws, ga)
        assert torch.equal(acc, pre + masked), "accumulate != pre + masked"
        record("conv", f"{route}-dgrad+accumulate", shape, marks)
    else:
        assert route in ("direct", "F2_gemm_f32")


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
def test_conv_dgrad_unpool_inside_its_workspace(ops, ws, accumulate):
    """the split-K data-gradient written through the pool's adjoint into a (27, 35) map: odd rows and columns outside every
    window.  Reference: the float64 data-gradient rounded once to float32 (2^-24 relative, far inside the direct route's 3e-6)
    and routed by strotss_maxpool2_bwd from the same codes, which copies values."""
    import test_hip_conv_routes as CR
    h, w, cin, cout, fh, fw = 13, 17, 256, 256, 27, 35
    assert ops.conv3x3_direct_splits(h, w, cout, cin)
    g = torch.Generator(device="cuda").manual_seed(77)
    wt = torch.randn(3, 3, cin, cout, generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    w_tik = wt.flip(0, 1).reshape(9, cin, cout).contiguous()
    gy = torch.randn(1, h, w, cout, generator=g, device="cuda")
    full = torch.randn(1, fh, fw, cin, generator=g, device="cuda")
    code = torch.empty((1, h, w, cin), dtype=torch.uint8, device="cuda")
    ops.maxpool2_fwd(full, code=code)
    ref_pooled = CR._conv64(gy, wt.flip(0, 1).transpose(2, 3))
    pre = torch.randn(1, fh, fw, cin, generator=g, device="cuda")
    want = ops.maxpool2_bwd(full, ref_pooled.float().contiguous(), code=code).double()
    if accumulate:
        want = want + pre.double()
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded((1, fh, fw, cin), F32, NAN, name="gin_full")
        if accumulate:
            out.copy_(pre)
        ops.conv3x3_dgrad_unpool(gy, w_tik, cin, code, out, accumulate=accumulate, ws=ws)
        marks = checked(ws, go)
        assert go.untouched() == 0
        mx, _ = CR._err(out, want)
        assert mx < CR.TOL["direct_splitk"], mx
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    record("conv", f"dgrad_unpool{'+accumulate' if accumulate else ''}", f"{h}x{w}x{cout}to{cin} into {fh}x{fw}", marks)


# ------------------------------------------------------------------ losses
LOSS_CASES = ("regime_small_n37", "step")            # the smallest ragged case (n 37, ns 300, d 2179); n = ns = 1024


def run_loss(ws, fn, n, d, scale, seed, written=((0, 1),), ld=None):
    """fn(gpred, loss (4, 4)) twice, each time from poisoned scratch into a guarded gradient buffer that holds a seeded base
    (the entries ADD) with the sentinel in its padding and into a guarded NaN loss buffer: guards, padding, the losses in
    `written` ((row, count) pairs) and only those, the same bits both times -> (added gradient float64 [:n, :d], losses
    float64, high-water marks)"""
    base = gpred_base(n, d, scale, seed)
    if ld is not None:                   # rows wider than the d columns the entry adds into: the rest is padding too
        wide = torch.full((base.shape[0], ld), float(base[-1, -1]) if base.shape[1] > d else 7.25, dtype=F32, device=DEV)
        wide[:n, :d] = base[:n, :d]
        base = wide
    runs = []
    for _ in range(2):
        ws.poison()
        gp, gg = SG.guarded(tuple(base.shape), F32, NAN, name="gpred")
        gp.copy_(base)
        lo, lg = SG.guarded((4, 4), F32, NAN, name="loss_out")
        fn(gp, lo)
        marks = checked(ws, gg, lg)
        assert torch.equal(gp[n:], base[n:]) and torch.equal(gp[:, d:], base[:, d:]), "padding of gpred changed"
        for row, count in written:
            assert lg.untouched(lo[row, :count]) == 0
        assert lg.untouched() == 16 - sum(count for _, count in written), "a loss slot outside the declared ones was written"
        runs.append((gp, lo))
    assert torch.equal(runs[0][0], runs[1][0]), "the second call from dirty scratch gives another gradient"
    assert torch.equal(runs[0][1].view(torch.int32), runs[1][1].view(torch.int32)), "... another loss"
    got = (gp.double() - base.double())[:n, :d].cpu().numpy()
    assert np.isfinite(got).all()
    return got, lo.double().cpu().numpy(), marks


def _col_weight(R):
    w = torch.zeros(LC_pad(R.c.n), dtype=F32, device=DEV)
    w[:R.c.n] = torch.as_tensor(R.col_weight, dtype=F32, device=DEV)
    return w


@pytest.fixture(scope="module", params=LOSS_CASES)
def R(request):
    import test_hip_loss_terms as LT
    return LT.refs_of(request.param)


def _shape(c):
    return f"n{c.n} ns{c.ns} d{c.d}"


@pytest.mark.parametrize("weighted", [False, True], ids=["plain", "weighted"])
def test_selfsim_inside_its_workspace(ops, ws, R, weighted):
    c = R.c
    l, g, b, _ = R.selfsim(weighted)
    by, bc, gs = fbuf(c.y), fbuf(c.c), 0.75
    cw = _col_weight(R) if weighted else None
    fn = lambda gp, lo: ops.selfsim_weighted_fwd_bwd(by, bc, cw, c.n, c.d, gs, gp, lo[0], ws=ws)
    got, loss, marks = run_loss(ws, fn, c.n, c.d, np.abs(g).max() * gs, 1)
    check_scalar("selfsim", c.label, loss[0, 0], l)
    check_gradient("selfsim_w" if weighted else "selfsim", c.label, got / gs, g, b)
    record("loss", "selfsim_weighted" if weighted else "selfsim", _shape(c), marks)


def test_moment_inside_its_workspace(ops, ws, R):
    import _loss_ref as LR
    c = R.c
    l, g, b, _ = R.moment()
    bx, by, gs = fbuf(c.x), fbuf(c.y), 1.5
    stats = []
    for _ in range(2):
        ws.poison()
        stats.append(ops.moment_stats(bx, c.ns, c.d, ws=ws))
        marks = checked(ws)
    mean, cov = stats[0]
    assert torch.equal(mean, stats[1][0]) and torch.equal(cov, stats[1][1])
    m64, S64 = LR.moment_stats(c.x)
    tc, tm = LR.cov_tau(c.x)
    assert (np.abs(cov[:c.d, :c.d].double().cpu().numpy() - S64) <= tc).all()
    assert (np.abs(mean[:c.d].double().cpu().numpy() - m64) <= tm).all()
    record("loss", "moment_stats", _shape(c), marks)
    fn = lambda gp, lo: ops.moment_fwd_bwd(mean, cov, by, c.n, c.d, gs, gp, lo[0], ws=ws)
    got, loss, marks = run_loss(ws, fn, c.n, c.d, np.abs(g).max() * gs, 2)
    check_scalar("moment", c.label, loss[0, 0], l)
    check_gradient("moment", c.label, got / gs, g, b)
    record("loss", "moment_fwd_bwd", _shape(c), marks)


@pytest.mark.parametrize("form", ["plain", "borrowed"])
def test_remd_inside_its_workspace(ops, ws, R, form):
    """borrowed: the selfsim call and the remd call that consumes its panels share the workspaces, nothing poisoned between"""
    c = R.c
    l, g, _, _ = R.remd("cos")
    bx, by, bc, gs = fbuf(c.x), fbuf(c.y), fbuf(c.c), 2.0
    panels = ops.row_inv_norm_x3(bx, c.ns)[1]
    rs = ops.row_inv_norm(bx, c.ns)
    before = dict(ops.remd_borrow_stats)

    def fn(gp, lo):
        if form == "borrowed":
            ops.selfsim_fwd_bwd(by, bc, c.n, c.d, 1.0, torch.zeros_like(by), lo[1], ws=ws)
            ops.remd_cos_fwd_bwd_after_selfsim(bx, rs, panels, c.ns, by, c.n, c.d, gs, gp, lo[0], ws=ws)
        else:
            ops.remd_cos_fwd_bwd(bx, rs, c.ns, by, c.n, c.d, gs, gp, lo[0], ws=ws)
    got, loss, marks = run_loss(ws, fn, c.n, c.d, np.abs(g).max() * gs, 3, ((0, 1), (1, 1)) if form == "borrowed" else ((0, 1),))
    if form == "borrowed":
        assert ops.remd_borrow_stats["borrowed"] == before["borrowed"] + 2 and ops.remd_borrow_stats["plain"] == before["plain"]
    check_scalar("remd_cos", c.label, loss[0, 0], l)
    check_gradient("remd_cos", c.label, got / gs, g)
    record("loss", f"remd_{form}", _shape(c), marks)


def test_palette_and_metric_remd_inside_their_workspaces(ops, ws, R):
    c = R.c
    bx, by = fbuf(c.x), fbuf(c.y)
    l, g, _, b = R.palette(True)
    got, loss, marks = run_loss(ws, lambda gp, lo: ops.palette_remd_fwd_bwd(bx, c.ns, by, c.n, 0.5, gp, lo[0], ws=ws),
                                c.n, c.d, np.abs(g).max() * 0.5, 4)
    check_scalar("palette", c.label, loss[0, 0], l)
    assert np.all(got[:, 3:] == 0.0)
    check_gradient("palette", c.label, got[:, :3] / 0.5, g, b)
    record("loss", "palette_remd", _shape(c), marks)
    for metric in ("l2", "both"):
        l, g, _, b = R.remd(metric)
        fn = lambda gp, lo: ops.remd_metric_fwd_bwd(bx, c.ns, by, c.n, c.d, metric, 1.25, gp, lo[0], ws=ws)
        got, loss, marks = run_loss(ws, fn, c.n, c.d, np.abs(g).max() * 1.25, 5)
        check_scalar(f"remd_{metric}", c.label, loss[0, 0], l)
        check_gradient(f"remd_{metric}", c.label, got / 1.25, g, b)
        record("loss", f"remd_metric_{metric}", _shape(c), marks)


@pytest.mark.parametrize("entry", ["step", "blend", "cw"])
def test_grouped_losses_inside_their_workspace(ops, ws, R, entry):
    """step_losses_fwd_bwd; step_losses_blend_fwd_bwd with the case's style twice at weights 0.4 and 0.3 (every per-style loss
    the single style's, the gradient 0.7 of its); step_losses_cw_fwd_bwd with column weights -- once per term, as
    tests/test_hip_loss_terms.py calls them"""
    import test_hip_loss_terms as LT
    assert ops.step_losses_available()
    c = R.c
    by, bc = fbuf(c.y), fbuf(c.c)
    t = LT._target(ops, c.x, c.ns, c.d)
    weighted = entry == "cw"
    cw = _col_weight(R) if weighted else None
    k_styles = 2 if entry == "blend" else 1
    wsum = sum(LC.BLEND_WEIGHTS[:2]) if entry == "blend" else 1.0
    s = ops.make_style_set([t] * k_styles, list(LC.BLEND_WEIGHTS[:2]) if entry == "blend" else [1.0])
    refs = [LT._term_ref(R, term, weighted and term == "content") for term in LT.TERMS]
    for k, term in enumerate(LT.TERMS):
        gv = [0.0] * 4
        gv[k] = LT.G_TERM[k]

        def fn(gp, lo):
            if entry == "step":
                ops.step_losses_fwd_bwd(by, bc, c.n, c.d, t.feats, t.inv_norm, t.panels, t.ns, t.mean, t.cov, *gv, gp,
                                        lo[0], lo[1], lo[2], lo[3], ws=ws)
            elif entry == "blend":
                ops.step_losses_blend_fwd_bwd(by, bc, c.n, c.d, s, *gv, gp, lo[0], lo[1], lo[2], lo[3], ws=ws)
            else:
                ops.step_losses_cw_fwd_bwd(by, bc, c.n, c.d, cw, s, *gv, gp, lo[0], lo[1], lo[2], lo[3], ws=ws)
        ref_l, ref_g, ref_b = refs[k]
        scale = 1.0 if term == "content" else wsum
        written = ((0, 1), (1, k_styles), (2, k_styles), (3, k_styles))
        got, loss, marks = run_loss(ws, fn, c.n, c.d, np.abs(ref_g).max() * LT.G_TERM[k] * scale, 10 + k, written)
        for kk in range(4):
            for si in range(k_styles if kk else 1):
                check_scalar(f"{entry}:{LT.TERMS[kk]}[{si}]", c.label, loss[kk, si], refs[kk][0])
        check_gradient(f"{entry}:{term}", c.label, got / LT.G_TERM[k], scale * ref_g, None if ref_b is None else scale * ref_b)
    record("loss", f"step_losses_{entry}", _shape(c), marks)


SK_LABEL = "n37_ns65"                    # tests/_sinkhorn_cases.py: n 37, ns 65, d 131, 30 iterations


@pytest.mark.parametrize("metric", ["cosine", "l2", "both"])
def test_sinkhorn_inside_its_workspace(ops, ws, metric):
    """strotss_sinkhorn_cos_fwd_bwd and strotss_sinkhorn_metric_fwd_bwd through test_hip_sinkhorn.py's entry (no ws=: the
    guarded instance stands at the module level)"""
    import _sinkhorn_cases as SC
    import _sinkhorn_ref as SR
    import test_hip_sinkhorn as TS
    c = SC.make_case(SK_LABEL)
    l = SR.l_of(SK_LABEL, metric)
    ref_l, ref_g = TS.ref64(SK_LABEL, metric)
    got, loss, marks = run_loss(ws, TS.entry(ops, c, metric, l, 0.37), c.n, c.d, np.abs(ref_g).max() * 0.37, 30)
    TS.check_loss(f"sinkhorn_{metric}", c, l, loss[0, 0], ref_l)
    TS.check_elements(f"sinkhorn_{metric}", SK_LABEL, got / 0.37, ref_g, SR.TOL_SK[SR.family(c, metric)])
    assert set(marks) == {next(iter(marks))} and next(iter(marks)).startswith("sinkhorn[")
    record("loss", f"sinkhorn_{metric}", _shape(c), marks)


def test_step_sinkhorn_inside_its_workspace(ops, ws):
    """strotss_sinkhorn_cos_fwd_bwd_panels after the content loss, through test_hip_transport.py's entry: the borrow, with
    nothing poisoned between the two calls"""
    import _sinkhorn_ref as SR
    import test_hip_transport as TT
    c, l = [(c, l) for c, l in TT.CASES if c.label == SK_LABEL][0]
    ref_l, ref_g = TT.ref64(SK_LABEL)
    got, loss, marks = run_loss(ws, TT.entry(ops, c, l, 0.37), c.n, c.d, np.abs(ref_g).max() * 0.37, 50)
    assert abs(loss[0, 0] - ref_l) / abs(ref_l) <= SR.loss_tolerance(c, l)
    tol = SR.TOL_SK[SR.family(c, "cosine")]
    assert (np.abs(got / 0.37 - ref_g) <= tol * np.abs(ref_g).max()).all(), SR.err_over_max(got / 0.37, ref_g)
    assert any(k.startswith("sinkhorn_step[") for k in marks) and any(k.startswith("selfsim[") for k in marks)
    record("loss", "sinkhorn_step", _shape(c), marks)


def test_log_sinkhorn_inside_its_workspace(ops, ws):
    """strotss_sinkhorn_log_cos_fwd_bwd_panels after the content loss at tests/_sinkhorn_log_cases.py's smallest case with
    both counts off the 64-row tiles (ns 63, n 65, d 35), through test_hip_sinkhorn_log.py's entry"""
    import _sinkhorn_log_cases as GC
    import _sinkhorn_log_ref as GR
    import test_hip_sinkhorn_log as TG
    c = GC.make_case("ns63_n65")
    ref_l, ref_g = TG.ref64(c.label)
    got, loss, marks = run_loss(ws, TG.entry(ops, c, c.l, c.T, 0.37), c.n, c.d, np.abs(ref_g).max() * 0.37, 70)
    assert abs(loss[0, 0] - ref_l) / abs(ref_l) <= GR.TOL_SCALAR
    tol = GR.TOL_SK[GR.family(c)]
    assert (np.abs(got / 0.37 - ref_g) <= tol * np.abs(ref_g).max()).all(), GR.err_over_max(got / 0.37, ref_g)
    assert any(k.startswith("sinkhorn_log_step[") for k in marks)
    record("loss", "sinkhorn_log_step", _shape(c), marks)


@pytest.mark.parametrize("label", ["n65_ns40_p4", "arc_n1024_ns1024_p4_wide"])   # smallest with both counts off the 64-row tile; n 1024
def test_sliced_inside_its_workspace(ops, ws, label):
    """strotss_sliced_cos_fwd_bwd through sliced_cos_fwd_bwd_after_selfsim: the content loss on the case's prediction rows
    first (its panels are borrowed), nothing poisoned between; the counter is a guarded int32 of its own.  Reference and
    bounds are test_hip_sliced.py::test_entry_matches_float64_element_by_element's."""
    import _sliced_cases as SC
    import _sliced_ref as SR
    import test_hip_sliced as TS
    from _sinkhorn_ref import loss_tolerance
    c = SC.make_case(label)
    ref_l, ref_g = TS.ref64(label)
    bx, by, gs = fbuf(c.x), fbuf(c.y), 0.37
    rs, xs = ops.row_inv_norm_x3(bx, c.ns)
    counter, gc = SG.guarded((1,), torch.int32, c.t, name="counter")

    def fn(gp, lo):
        counter.fill_(c.t)
        ops.selfsim_fwd_bwd(by, by, c.n, c.d, 1.0, torch.zeros_like(by), lo[1], ws=ws)
        ops.sliced_cos_fwd_bwd_after_selfsim(bx, rs, xs, c.ns, by, c.n, c.d, c.n_proj, c.seed, counter, gs, gp, lo[0], ws=ws)
    got, loss, marks = run_loss(ws, fn, c.n, c.d, max(np.abs(ref_g).max(), 1e-3) * gs, 80, ((0, 1), (1, 1)))
    gc.check()
    assert int(counter.item()) == c.t + 1
    assert abs(loss[0, 0] - ref_l) / abs(ref_l) <= loss_tolerance(c, 0.0)
    tol = SR.TOL_GRAD[SR.family(c)]
    assert (np.abs(got / gs - ref_g) <= tol * np.abs(ref_g).max()).all(), SR.err_over_max(got / gs, ref_g)
    assert any(k.startswith("sliced_step[") for k in marks) and any(k.startswith("selfsim[") for k in marks)
    record("loss", "sliced", f"n{c.n} ns{c.ns} d{c.d} P{c.n_proj}", marks)


@pytest.mark.parametrize("label", ["n65_ns33_p8", "line_n1024_ns1024_p8"])       # smallest ragged (rows 2208 wide); n 1024
def test_palette_sliced_inside_its_workspace(ops, ws, label):
    """reference and bounds are test_hip_palette_sliced.py::test_entry_matches_float64_element_by_element's"""
    import _palette_sliced_cases as PC
    import _palette_sliced_ref as PR
    import test_hip_palette_sliced as TP
    c = PC.make_case(label)
    ref_l, ref_g = TP.ref64(label)
    style, pred, gs = TP.rows(c.x, c.ld), TP.rows(c.y, c.ld), 0.37
    dirs = torch.from_numpy(c.dirs).to(DEV).contiguous()
    fn = lambda gp, lo: ops.palette_sliced_fwd_bwd(style, c.ns, pred, c.n, dirs, gs, gp, lo[0], rgb_to_yuv=c.rgb_to_yuv, ws=ws)
    got, loss, marks = run_loss(ws, fn, c.n, 3, max(np.abs(ref_g).max(), 1e-3) * gs, 90, ld=c.ld)
    assert abs(loss[0, 0] - ref_l) / abs(ref_l) <= PR.LOSS_TOL
    tol = PR.TOL_GRAD[PR.family(c)]
    assert (np.abs(got / gs - ref_g) <= tol * np.abs(ref_g).max()).all(), PR.err_over_max(got / gs, ref_g)
    assert set(marks) == {next(iter(marks))} and next(iter(marks)).startswith("palette_sliced[")
    record("loss", "palette_sliced", f"n{c.n} ns{c.ns} ld{c.ld} P{c.n_proj}", marks)


# ------------------------------------------------------------------ the pixel side
def _img(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=F32, device=DEV)


@pytest.mark.parametrize("label", ["1x1", "3x8193"])          # the case module's smallest; both sides odd, 97 reduction blocks
def test_tv_inside_its_workspace(ops, ws, label):
    import _pixel_prior_cases as PC
    import _pixel_prior_ref as PR
    from nn import _hip
    P = PC.tv_inputs(label)
    h, w, gs = P["h"], P["w"], 1.5
    nb = int(_hip.lib().strotss_tv_workspace_bytes(h, w))
    ref_l, ref_g = PR.tv(P["x"], gscale=gs)
    xd, runs = _img(P["x"]), []
    for _ in range(2):
        ws.poison()
        g, gg = SG.guarded((h, w, 3), F32, NAN, name="gimg")
        g.copy_(_img(P["g0"]))
        loss, lg = SG.guarded((4,), F32, NAN, name="loss_out")
        ops.tv_fwd_bwd(xd, gs, g, loss, ws.zeroed("tv", (h, w), nb, DEV))
        marks = checked(ws, gg, lg)
        assert lg.untouched() == 3 and lg.untouched(loss[:1]) == 0
        runs.append((g, loss))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1][:1], runs[1][1][:1])
    got_g = g.double().cpu().numpy() - P["g0"].astype(np.float64)
    scale = float(np.abs(ref_g).max())
    ulp = 2.0 ** -23 * float((np.abs(P["g0"]).astype(np.float64) + np.abs(ref_g)).max())      # the one float32 addition to g0
    err = float(np.abs(got_g - ref_g).max())
    rel = abs(loss[0].item() - float(ref_l)) / abs(float(ref_l)) if abs(float(ref_l)) > 1e-15 else abs(loss[0].item())
    assert rel <= PR.LOSS_TOL and err <= PR.TOL_GRAD["tv"] * scale + ulp, (rel, err, scale)
    record("pixel", "tv_fwd_bwd", label, marks)


@pytest.mark.parametrize("label", ["1x1-p1-absent", "33x65-p2_16-absent"])
def test_detail_inside_its_workspace(ops, ws, label):
    import _pixel_prior_cases as PC
    import _pixel_prior_ref as PR
    from nn import _hip
    P = PC.detail_inputs(label)
    h, w, pools = P["h"], P["w"], P["pools"]
    gs = [1.5, 0.5, 2.0][:len(pools)]
    nb = int(_hip.lib().strotss_detail_workspace_bytes(h, w))
    ref_l, ref_g = PR.detail(P["x"], P["c"], pools, P["weights"], gs)
    xd, cd = _img(P["x"]), _img(P["c"])
    contents = [ops.pool_mean(cd, p) for p in pools]
    cells = [None if m is None else _img(m) for m in P["weights"]]
    runs = []
    for _ in range(2):
        ws.poison()
        g, gg = SG.guarded((h, w, 3), F32, NAN, name="gimg")
        g.copy_(_img(P["g0"]))
        loss, lg = SG.guarded((4,), F32, NAN, name="loss_out")
        ops.detail_fwd_bwd(xd, pools, contents, cells, gs, g, loss, ws.zeroed("detail", (h, w), nb, DEV))
        marks = checked(ws, gg, lg)
        assert lg.untouched() == 4 - len(pools) and lg.untouched(loss[:len(pools)]) == 0
        runs.append((g, loss))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1][:len(pools)], runs[1][1][:len(pools)])
    got_g = g.double().cpu().numpy() - P["g0"].astype(np.float64)
    scale = float(np.abs(ref_g).max())
    ulp = 2.0 ** -23 * float((np.abs(P["g0"]).astype(np.float64) + np.abs(ref_g)).max())      # one float32 addition per pool
    err = float(np.abs(got_g - ref_g).max())
    got_l = loss[:len(pools)].double().cpu().numpy()
    rel = max((abs(a - float(b)) / abs(float(b)) if float(b) != 0 else abs(a)) for a, b in zip(got_l, ref_l))
    assert rel <= PR.LOSS_TOL and err <= PR.TOL_GRAD[PR.family(pools)] * scale + len(pools) * ulp, (rel, err, scale)
    record("pixel", "detail_fwd_bwd", label, marks)


@pytest.mark.parametrize("hw", [(1, 1), (33, 65)])             # test_hip_smooth.py's smallest shape; both sides odd
def test_guided_smooth_inside_its_workspace(ops, ws, hw):
    import _smooth_ref as SMR
    (h, w), r, eps = hw, 4, 1e-2
    p, I = SMR.test_images(h, w, 1000 * r + h + w)
    pd, Id = _img(p), _img(I)
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded((h, w, 3), F32, NAN, name="out")
        ops.guided_smooth(pd, Id, r, eps, out=out, ws=ws)
        marks = checked(ws, go)
        assert go.untouched() == 0
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref = SMR.guided_separable(p, I, r, eps, full=True)
    e_round, e_stat = SMR.error_budgets(p, I, r, eps, ref)
    assert (np.abs(out.double().cpu().numpy() - ref["q"]) <= e_round + e_stat).all()
    record("pixel", "guided_smooth", f"{h}x{w} r{r}", marks)


@pytest.mark.parametrize("hw", [(1, 3), (33, 65)])             # test_hip_temporal_long.py's smallest; both sides odd, three partials
@pytest.mark.parametrize("count", [1, 4])
def test_temporal_inside_its_workspace(ops, ws, hw, count):
    """count 1 through temporal_fwd_bwd, count 4 through temporal_multi_fwd_bwd; reference and bound (1e-5 of the loss and of
    the largest gradient element) are test_hip_temporal_long.py::test_multi_fwd_bwd_matches_float64's"""
    import _temporal_long_ref as TL
    import test_hip_temporal_long as TT
    from nn import _hip
    h, w = hw
    x, tg, cs, g0 = TT._multi_inputs(h, w, count, h + w + count)
    gs = [3.5, 0.75, 12.0, 2.0][:count]
    xd, tds, cds = _img(x), [_img(t) for t in tg], [_img(c) for c in cs]
    nb = int(_hip.lib().strotss_temporal_multi_workspace_bytes(h, w, count))
    runs = []
    for _ in range(2):
        ws.poison()
        g, gg = SG.guarded((h, w, 3), F32, NAN, name="gimg")
        g.copy_(_img(g0))
        loss, lg = SG.guarded((4,), F32, NAN, name="loss_out")
        scratch = ws.zeroed("temporal", (h, w, count), nb, DEV)
        if count == 1:
            ops.temporal_fwd_bwd(xd, tds[0], cds[0], gs[0], g, loss, scratch)
        else:
            ops.temporal_multi_fwd_bwd(xd, tds, cds, gs, g, loss, scratch)
        marks = checked(ws, gg, lg)
        assert lg.untouched() == 4 - count and lg.untouched(loss[:count]) == 0
        runs.append((g, loss))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1][:count], runs[1][1][:count])
    ref_l, ref_g = TL.multi_loss64(xd.cpu().double().numpy(), [t.cpu().double().numpy() for t in tds],
                                   [c.cpu().double().numpy() for c in cds], gs)
    ref_g = g0.astype(np.float64) + ref_g
    got_l = loss[:count].cpu().double().numpy()
    for j in range(count):
        assert abs(got_l[j] - ref_l[j]) <= 1e-5 * abs(ref_l[j]), (j, got_l[j], ref_l[j])
    got = g.cpu().double().numpy()
    assert float(np.abs(got - ref_g).max()) <= 1e-5 * float(np.abs(ref_g).max())
    none = np.all([c == 0 for c in cs], axis=0)                  # no certainty for any j: the base, untouched
    assert np.array_equal(got[none], g0[none].astype(np.float64))
    record("pixel", "temporal_fwd_bwd" if count == 1 else "temporal_multi_fwd_bwd", f"{h}x{w} count {count}", marks)


@pytest.mark.parametrize("mode", ["guided", "residual"])
@pytest.mark.parametrize("lo,hi", [((1, 1), (3, 5)), ((33, 65), (67, 131))])   # test_hip_upsample.py's smallest; all sides odd
def test_guided_upsample_inside_its_workspace(ops, ws, lo, hi, mode):
    """reference and per-element budget are test_hip_upsample.py::test_guided_upsample_matches_float64's"""
    import _upsample_ref as UR
    r, eps = 4, 1e-2
    p, I_lo, I_hi = UR.test_images(*lo, *hi, 1000 * r + lo[0] + hi[1])
    pd, lod, hid = _img(p), _img(I_lo), _img(I_hi)
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded(hi + (3,), F32, NAN, name="out")
        ops.guided_upsample(pd, lod, hid, r, eps, mode, out=out, ws=ws)
        marks = checked(ws, go)
        assert go.untouched() == 0
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    ref = UR.coefficients(p, I_lo, r, eps)
    want = UR.upsample(p, I_lo, I_hi, r, eps, mode, ref=ref)
    e_round, e_stat = UR.error_budgets(p, I_lo, I_hi, r, eps, mode, ref)
    assert (np.abs(out.double().cpu().numpy() - want) <= e_round + e_stat).all()
    record("pixel", f"guided_upsample {mode}", f"{lo[0]}x{lo[1]} to {hi[0]}x{hi[1]} r{r}", marks)


@pytest.mark.parametrize("cid", ["one_blocked_launch-2x2", "one_blocked_launch-37x75"])    # the entry's minimum; odd by odd, two
def test_optical_flow_inside_its_workspace(ops, ws, cid):                                  # tiles wide and high, two levels
    """reference and bound (F32_YARDSTICK x the float32 restatement's own distance) are test_hip_flow.py::
    test_stage_sets_match_float64's"""
    import _flow_cases as FC
    import test_hip_flow as TF
    _, h, w, seed, params = [c for c in FC.stage_cases() if c[0] == cid][0]
    a, b = FC.frames(h, w, seed)
    f64, yard = FC.reference(h, w, seed, params)
    ad, bd, prm = _img(a), _img(b), ops.flow_params(**params)
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded((h, w, 2), F32, NAN, name="flow")
        ops.optical_flow(ad, bd, prm, out=out, ws=ws)
        marks = checked(ws, go)
        assert go.untouched() == 0
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    TF._against_float64(cid, out.cpu().numpy(), f64, yard)
    record("pixel", "optical_flow", cid, marks)


@pytest.mark.parametrize("kind", [None, "random"])
@pytest.mark.parametrize("hw", [(1, 1), (33, 65)])             # test_hip_color.py's smallest; both sides odd
def test_color_stats_inside_its_workspace(ops, ws, hw, kind):
    """reference and bound (N 2^-53 relative) are test_hip_color.py::test_color_stats_matches_float64's"""
    import _color_ref as CRF
    import test_hip_color as TC
    h, w = hw
    x, m = TC._image(h, w, h + w), TC._mask(kind, h, w)
    xd, md = _img(x), None if m is None else _img(m)
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded((10,), torch.float64, NAN, name="sums")
        ops.color_stats(xd, md, ws=ws, out=out)
        marks = checked(ws, go)
        assert go.untouched() == 0
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int64), outs[1].view(torch.int64))
    got, ref = out.cpu().numpy(), CRF.sums64(x, m, exact=True)
    assert (np.abs(got - ref) <= h * w * 2.0 ** -53 * np.abs(ref)).all(), (got, ref)
    record("pixel", "color_stats", f"{h}x{w} mask {kind}", marks)


@pytest.mark.parametrize("shape", [(1, 1, 1), (33, 65, 4)])    # _detail_map_ref's smallest; both sides odd
def test_detail_map_inside_its_workspace(ops, ws, shape):
    """reference and bound (4 E32 + 1e-7) are test_hip_detail_map.py::test_device_map_against_float64's"""
    import _detail_map_ref as DR
    h, w, r = shape
    gain, floor = DR.PARAMS[0]
    img, ref, _, e32 = DR.case("random", shape, (gain, floor))
    xd = _img(img)
    outs = []
    for _ in range(2):
        ws.poison()
        out, go = SG.guarded((h, w), F32, NAN, name="map")
        ops.detail_map(xd, r, gain, floor, ws=ws, out=out)
        marks = checked(ws, go)
        assert go.untouched() == 0
        outs.append(out)
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))
    got = out.double().cpu().numpy()
    assert np.isfinite(got).all() and float(np.abs(got - ref).max()) <= 4.0 * e32 + 1e-7
    record("pixel", "detail_map", f"{h}x{w} r{r}", marks)


@pytest.mark.parametrize("case", [(1, 2, 2), (33, 67, 7)], ids=lambda c: "%dx%d-k%d" % c)   # _scribble_cases' smallest; odd by
def test_scribble_labels_inside_its_workspace(ops, ws, case):                              # odd, above the 32 x 64 tile
    """reference and bound (BOUND_FACTOR x Y) are test_hip_scribble.py::test_blocked_equals_plain_and_both_match_float64's,
    at the case's largest sweep count"""
    import _scribble_cases as S
    import _scribble_ref as R
    import test_hip_scribble as TSC
    h, w, k = case
    n = S.sweeps_of((h, w))[-1]
    img, stroke, scores = (torch.as_tensor(np.ascontiguousarray(a), dtype=t, device=DEV)
                           for a, t in zip(S.make(h, w, k), (F32, torch.int32, F32)))
    ref, Y = S.run(h, w, k)[n], S.yardstick(h, w, k, n)
    outs = []
    for _ in range(2):
        ws.poison()
        label, gl = SG.guarded((h, w), torch.int32, 0x7FC0BEEF, name="label")
        count, gn = SG.guarded((k,), torch.int32, 0x7FC0BEEF, name="count")
        x, gx = SG.guarded((k, h, w), F32, NAN, name="planes")
        ops.scribble_labels(img, stroke, scores, R.TAU, R.LAMBDA, R.SIGMA, n, 0, planes=True, ws=ws, out=(label, count, x))
        marks = checked(ws, gl, gn, gx)
        assert gl.untouched() == 0 and gn.untouched() == 0 and gx.untouched() == 0
        outs.append((label, count, x))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(*outs))
    label, count, x = (t.cpu().numpy() for t in outs[1])
    assert (np.abs(x.astype(np.float64) - ref["x"]) <= TSC.BOUND_FACTOR * Y).all()
    wide = ref["margin"] >= S.MARGIN_FACTOR * Y
    assert np.array_equal(label[wide], ref["label"][wide])
    assert np.array_equal(count, np.bincount(label.reshape(-1), minlength=k))
    record("pixel", "scribble_labels", f"{h}x{w} k{k} {n} sweeps", marks)


# ------------------------------------------------------------------ the engine
@pytest.mark.parametrize("transport", ["remd", "sinkhorn", "pixel_terms"])
def test_engine_inside_its_workspaces_eager_captured_and_replayed(ops, monkeypatch, transport):
    """the product's real sequence of tags and sizes -- one tag asked for different sizes by different layers, the borrow, the
    frozen arena -- on exact buffers: three eager steps, capture, three replays; guards after each phase; variables,
    gradients and scalars bit for bit those of the same run on nn._ops.Workspaces.  "pixel_terms": _pixel_terms_cases'
    42 x 64 engine with two temporal targets, the detail term with a cell map, TV and the photo term: their four zeroed
    workspaces are blocks of the engine's instance, each of exactly the library's byte count, and the terms' scalars are
    compared as well"""
    import _pixel_terms_cases as TPP
    import test_hip_workspaces as TW
    terms = transport == "pixel_terms"
    P = None if terms else TR.step_problem(TW.H, TW.W, TW.N, 21)
    idx = TPP.all_terms_indices(3) if terms else TW._indices(3, 6)
    zeroed = {}

    def run(guard):
        with monkeypatch.context() as m:
            if guard:
                m.setattr(ops, "Workspaces", SG.GuardedWorkspaces)
            eng = TPP.all_terms_engine() if terms else TW._engine(P, transport=transport, deterministic=True)
        if guard:
            zeroed.update({(tag, key): blk.nbytes for (tag, _, key), blk in eng._ws.fixed_blocks.items()})
        assert isinstance(eng._ws, SG.GuardedWorkspaces) == guard and eng.trunk.ws is eng._ws
        out, marks = [], {}
        phase = lambda: checked(eng._ws) if guard else torch.cuda.synchronize()
        for i in idx:
            eng.step(i)
            out.append(eng.scalars.clone())
        phase()
        eng.capture_graph(idx[0])
        phase()
        assert eng._graph is not None and eng._ws.frozen
        for i in idx:
            eng.step(i)
            out.append(eng.scalars.clone())
        marks = phase()
        return out + [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + \
            [t.loss.clone() for t in eng._pixel_terms], marks
    guarded, marks = run(True)
    plain, _ = run(False)
    assert len(guarded) == len(plain) == 6 + 6 + 6 + (4 if terms else 0)
    for a, b in zip(guarded, plain):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert len({k.split("[")[0] for k in marks}) < len(marks), "no tag was asked for two sizes: not the trunk's sequence"
    if terms:
        from nn import _hip
        (h, w), lib = TPP.ALL_TERMS_HW, _hip.lib()
        assert zeroed == {("temporal", (h, w, 2)): lib.strotss_temporal_multi_workspace_bytes(h, w, 2),
                          ("detail", (h, w)): lib.strotss_detail_workspace_bytes(h, w),
                          ("tv", (h, w)): lib.strotss_tv_workspace_bytes(h, w),
                          ("matting", (h, w)): lib.strotss_matting_workspace_bytes(h, w)}
        record("engine", "StepEngine pixel terms", f"{h}x{w} n300", marks)
    else:
        record("engine", f"StepEngine {transport}", f"{TW.H}px n{TW.N}", marks)
