"""The loss GEMMs' maps from workgroup id to output tile (csrc/gemm.hip, csrc/mfma_x3.h) at every tile grid, against float64
(tests/_tilegrid_cases.py holds the cases; DESIGN.md section 6, 'Tile-grid sweeps', the measured values).

1. strotss_cosine_distance_x3 / strotss_cosine_distance at every (g, gs) in 1..16 x 1..33 in three edge variants, called
   through the library into a sentinel-filled C of (nx + 8, pad32(ny) + 32): every element of [0, nx) x [0, ny) written and
   within EPS_COST of float64, every other element -- rows past nx AND the pad columns ny .. ldc - 1, which neither
   epilogue writes (include/strotss_hip.h) -- the sentinel, bit for bit; x == y: bitwise symmetric, diagonal within EPS_COST of 0.
2. strotss_step_losses_fwd_bwd against the four separate entries at 64 (n, ns) pairs, bit for bit; the blended call against
   the separate entries at k = 1..4 styles (k = 1 bit for bit, k > 1 within the stated 1e-5).
3. strotss_moment_stats at ceil(ld / 128) = 1..18: bitwise symmetric, every element within the derived bound
   (_tilegrid_cases.cov_bound), nothing written past the ld x ld matrix; strotss_moment_fwd_bwd's loss at the same widths."""
import numpy as np
import pytest
import torch

import _loss_ref as LR
import _tilegrid_cases as TG
from _loss_harness import DEV, fbuf, report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


def _lib():
    from nn import _hip
    return _hip, _hip.lib()


# ------------------------------------------------------------------ 1. the cosine products
class Sweep:
    """device side of the cosine sweep: the two row matrices, their float64 references, one output buffer, and the x3
    panels per distinct row count (the plane stride of a panel IS its row count)"""

    def __init__(self, ops):
        pred, style = TG.sweep_rows()
        cross, self_ = TG.sweep_refs()
        self.ops = ops
        self.rows = {"p": fbuf(pred), "s": fbuf(style)}
        self.ld = int(self.rows["p"].shape[1])
        assert self.ld == 64
        self.r = {"p": ops.row_inv_norm(self.rows["p"], TG.N_PRED), "s": ops.row_inv_norm(self.rows["s"], TG.N_STYLE)}
        self.cross = torch.as_tensor(np.array(cross), device=DEV)        # (a copy: the shared reference is read-only)
        self.self_ = torch.as_tensor(np.array(self_), device=DEV)
        self.cbuf = torch.empty((TG.N_PRED + TG.C_EXTRA_ROWS) * (TG.pad32(TG.N_STYLE) + TG.C_EXTRA_COLS), dtype=torch.int32,
                                device=DEV)
        self._panels = {}

    def panels(self, side, n):
        if (side, n) not in self._panels:
            self._panels[(side, n)] = self.ops.row_inv_norm_x3(self.rows[side], n)
        return self._panels[(side, n)]

    def launch(self, core, xside, nx, yside, ny):
        """one launch into the sentinel-filled buffer -> (C as int32 bits, C as f32), both (nx + 8, ldc)"""
        _hip, lib = _lib()
        ldc = TG.pad32(ny) + TG.C_EXTRA_COLS
        bits = self.cbuf[:(nx + TG.C_EXTRA_ROWS) * ldc].view(nx + TG.C_EXTRA_ROWS, ldc)
        bits.fill_(TG.SENTINEL_BITS)
        if core == "x3":
            rx, px = self.panels(xside, nx)
            ry, py = (rx, px) if (xside == yside and nx == ny) else self.panels(yside, ny)
            _hip.check(lib.strotss_cosine_distance_x3(px.data_ptr(), rx.data_ptr(), nx, py.data_ptr(), ry.data_ptr(), ny, self.ld,
                                                      bits.data_ptr(), ldc, _hip.stream_ptr()), "cosine_distance_x3")
        else:
            _hip.check(lib.strotss_cosine_distance(self.rows[xside].data_ptr(), self.r[xside].data_ptr(), nx,
                                                   self.rows[yside].data_ptr(), self.r[yside].data_ptr(), ny, self.ld,
                                                   bits.data_ptr(), ldc, _hip.stream_ptr()), "cosine_distance")
        return bits, bits.view(torch.float32)

    def measure(self, bits, vals, nx, ny, ref):
        """on the device: [unwritten elements of the region, worst |C - ref| there (inf where not a number), elements changed
        in the rows past nx, elements changed in the pad columns]"""
        err = torch.nan_to_num((vals[:nx, :ny].double() - ref[:nx, :ny]).abs(), nan=float("inf")).max()
        return torch.stack([(bits[:nx, :ny] == TG.SENTINEL_BITS).sum().double(), err,
                            (bits[nx:] != TG.SENTINEL_BITS).sum().double(), (bits[:nx, ny:] != TG.SENTINEL_BITS).sum().double()])


@pytest.fixture(scope="module")
def sweep(ops):
    return Sweep(ops)


def _assert_region(what, labels, got):
    """got: (cases, 4) of Sweep.measure; the worst figures are printed before anything is asserted"""
    worst = int(np.argmax(got[:, 1]))
    report(f"tilegrid_cost_err:{what}", labels[worst], f"{got[worst, 1]:.3e} of EPS_COST {LR.EPS_COST:.1e}")
    for k, name in ((0, "elements of [0, nx) x [0, ny) never written"), (2, "elements written in the rows past nx"),
                    (3, "elements written in the pad columns ny .. ldc - 1")):
        bad = [(labels[i], int(got[i, k])) for i in np.nonzero(got[:, k])[0]]
        assert not bad, (what, name, bad[:8], len(bad))
    bad = [(labels[i], float(got[i, 1])) for i in np.nonzero(~(got[:, 1] <= LR.EPS_COST))[0]]
    assert not bad, (what, "beyond EPS_COST of float64", bad[:8], len(bad))


@pytest.mark.parametrize("variant", TG.VARIANTS)
@pytest.mark.parametrize("core", ["x3", "f32"])
def test_cosine_distance_at_every_grid(sweep, core, variant):
    cases = TG.cosine_cases(variant)
    out = []
    for g, gs, n, ns in cases:
        bits, vals = sweep.launch(core, "p", n, "s", ns)
        out.append(sweep.measure(bits, vals, n, ns, sweep.cross))
    got = torch.stack(out).cpu().numpy()
    _assert_region(f"{core}:{variant}", [f"g{g}_gs{gs}_n{n}_ns{ns}" for g, gs, n, ns in cases], got)


@pytest.mark.parametrize("core", ["x3", "f32"])
def test_symmetric_cosine_distance_at_every_g(sweep, core):
    cases = TG.symm_cases()
    out, sym = [], []
    for variant, g, n in cases:
        bits, vals = sweep.launch(core, "p", n, "p", n)
        out.append(sweep.measure(bits, vals, n, n, sweep.self_))
        D = bits[:n, :n]
        sym.append(torch.stack([(D != D.T).sum().double(), torch.nan_to_num(vals[:n, :n].diagonal().abs(), nan=float("inf")).max().double()]))
    got, sym = torch.stack(out).cpu().numpy(), torch.stack(sym).cpu().numpy()
    labels = [f"{v}_g{g}_n{n}" for v, g, n in cases]
    report(f"tilegrid_symm_diag:{core}", labels[int(np.argmax(sym[:, 1]))], f"{sym[:, 1].max():.3e}")
    _assert_region(f"{core}:symm", labels, got)
    bad = [(labels[i], int(sym[i, 0])) for i in np.nonzero(sym[:, 0])[0]]
    assert not bad, (core, "D != D.T bitwise", bad)
    bad = [(labels[i], float(sym[i, 1])) for i in np.nonzero(~(sym[:, 1] <= LR.EPS_COST))[0]]
    assert not bad, (core, "diagonal beyond EPS_COST of 0", bad)


# ------------------------------------------------------------------ 2. the grouped launches
class Group:
    """zero-padded device buffers of the leading rows of _tilegrid_cases.group_rows(), and the style side per row count"""

    def __init__(self, ops):
        self.ops = ops
        self.y, self.c, self.x = TG.group_rows()
        self._pred, self._style = {}, {}

    def pred(self, n):
        if n not in self._pred:
            self._pred[n] = (fbuf(self.y[:n]), fbuf(self.c[:n]))
        return self._pred[n]

    def style(self, ns):
        if ns not in self._style:
            from nn.engine import StyleTarget
            self._style[ns] = StyleTarget.build(fbuf(self.x[:ns]), ns, TG.D_GROUP)
        return self._style[ns]

    def separate(self, n, targets, weights):
        """the engine's separate path: the content entry once, then per style moment, relaxed EMD (on the panels the content
        entry left) and palette with g * w_k -> (gpred, content loss (1,), per-style losses (3, k))"""
        ops, d = self.ops, TG.D_GROUP
        by, bc = self.pred(n)
        g = torch.zeros_like(by)
        lc = torch.zeros(4, device=DEV)
        per = torch.zeros((3, 4), device=DEV)
        gc, gm, gr, gp = TG.GROUP_G
        ops.selfsim_fwd_bwd(by, bc, n, d, gc, g, lc)
        for k, (t, w) in enumerate(zip(targets, weights)):
            ops.moment_fwd_bwd(t.mean, t.cov, by, n, d, gm * w, g, per[0, k:])
            ops.remd_cos_fwd_bwd_after_selfsim(t.feats, t.inv_norm, t.panels, t.ns, by, n, d, gr * w, g, per[1, k:])
            ops.palette_remd_fwd_bwd(t.feats, t.ns, by, n, gp * w, g, per[2, k:])
        torch.cuda.synchronize()
        return g, lc[:1].clone(), per[:, :len(targets)].clone()


@pytest.fixture(scope="module")
def group(ops):
    if not ops.step_losses_available():
        pytest.skip("bf16x3 core switched off")
    return Group(ops)


@pytest.mark.parametrize("n", TG.GROUP_N)
def test_grouped_step_losses_equal_the_separate_entries_bitwise(group, n):
    """the three forward products in one grouped launch (gemm_x3_group3_kernel: covariance | symmetric pair | full cost grid at
    pad8-aligned offsets, the third with its own XCD blocking) == the four separate entries, at every ns of the sweep"""
    ops, d = group.ops, TG.D_GROUP
    by, bc = group.pred(n)
    gc, gm, gr, gp = TG.GROUP_G
    bad = []
    for ns in TG.GROUP_NS:
        t = group.style(ns)
        borrowed = ops.remd_borrow_stats["borrowed"]
        gs, lc, per = group.separate(n, [t], [1.0])
        assert ops.remd_borrow_stats["borrowed"] == borrowed + 1           # the panels path: the third problem's own launch
        g = torch.zeros_like(by)
        l = torch.zeros(4, device=DEV)
        ops.step_losses_fwd_bwd(by, bc, n, d, t.feats, t.inv_norm, t.panels, ns, t.mean, t.cov, gc, gm, gr, gp, g, l[0:], l[1:],
                                l[2:], l[3:])
        torch.cuda.synchronize()
        want = torch.cat([lc, per[:, 0]])
        kind = TG.host_block(TG.tiles(n), TG.tiles(ns))[2]
        if not (torch.equal(l, want) and torch.equal(g, gs)):
            bad.append((n, ns, kind, l.tolist(), want.tolist(), int((g != gs).any(1).sum())))
        # (one prediction row: its self-similarity matrix is the single entry 0, the content loss with it)
        assert all(np.isfinite(float(v)) and (float(v) != 0.0 or (n == 1 and i == 0)) for i, v in enumerate(want)), (n, ns, want)
        assert float(gs[n:].abs().sum()) == 0.0 and float(gs[:, d:].abs().sum()) == 0.0
    assert not bad, bad


@pytest.mark.parametrize("n,ns", TG.BLEND_CASES, ids=[f"n{n}_k{len(ns)}" for n, ns in TG.BLEND_CASES])
def test_blended_step_losses_equal_the_separate_entries(group, n, ns):
    """gemm_x3_group_set_kernel (one cost problem per style, each at a pad8-aligned offset with its own blocking) against the
    separate entries: one style IS the single-style call (bit for bit); several: losses and gradient within BLEND_TOL"""
    ops, d = group.ops, TG.D_GROUP
    by, bc = group.pred(n)
    k = len(ns)
    targets = [group.style(s) for s in ns]
    weights = [1.0] if k == 1 else list(TG.BLEND_WEIGHTS[:k])
    gs, lc, per = group.separate(n, targets, weights)
    g = torch.zeros_like(by)
    out = torch.zeros((4, 4), device=DEV)
    gc, gm, gr, gp = TG.GROUP_G
    ops.step_losses_blend_fwd_bwd(by, bc, n, d, ops.make_style_set(targets, weights), gc, gm, gr, gp, g, out[0], out[1], out[2],
                                  out[3])
    torch.cuda.synchronize()
    got_c, got = out[0, :1], out[1:, :k]
    scale = float(gs.abs().max())
    dg = float((g - gs).abs().max()) / scale
    dl = float(((got - per).abs() / per.abs().clamp(min=1.0)).max())
    dc = abs(float(got_c) - float(lc)) / max(1.0, abs(float(lc)))
    report("tilegrid_blend", f"n{n}_ns{'_'.join(map(str, ns))}", f"grad {dg:.3e} losses {dl:.3e} content {dc:.3e}")
    assert scale > 0 and bool(torch.isfinite(g).all()) and bool((per != 0).all())
    if k == 1:
        assert torch.equal(got_c, lc) and torch.equal(got, per) and torch.equal(g, gs)
    else:
        assert dc <= TG.BLEND_TOL and dl <= TG.BLEND_TOL and dg <= TG.BLEND_TOL, (dc, dl, dg)
    assert float(g[n:].abs().sum()) == 0.0 and float(g[:, d:].abs().sum()) == 0.0


# ------------------------------------------------------------------ 3. the triangular covariance grid
MOMENT_TAIL = 4096


@pytest.mark.parametrize("d", TG.MOMENT_D)
def test_moment_stats_at_every_triangular_grid(ops, d):
    _hip, lib = _lib()
    n = TG.MOMENT_N
    x, y = TG.moment_rows(d)
    bx, by = fbuf(x), fbuf(y)
    ld = int(bx.shape[1])
    nb = int(lib.strotss_moment_workspace_bytes(n, ld))
    ws = ops.workspaces.get("moment", nb, bx.device)
    cov_bits = torch.full((ld * ld + MOMENT_TAIL,), TG.SENTINEL_BITS, dtype=torch.int32, device=DEV)
    mean_bits = torch.full((ld + MOMENT_TAIL,), TG.SENTINEL_BITS, dtype=torch.int32, device=DEV)
    _hip.check(lib.strotss_moment_stats(bx.data_ptr(), n, d, ld, mean_bits.data_ptr(), cov_bits.data_ptr(), ws.data_ptr(), nb,
                                        _hip.stream_ptr()), "moment_stats")
    torch.cuda.synchronize()
    cb = cov_bits[:ld * ld].view(ld, ld)
    cov, mean = cb.view(torch.float32), mean_bits[:ld].view(torch.float32)
    m64, S64 = LR.moment_stats(x)
    bc, bm = TG.cov_bound(x, TG.pad32(n))
    ec = np.abs(cov[:d, :d].double().cpu().numpy() - S64)
    em = np.abs(mean[:d].double().cpu().numpy() - m64)
    report("tilegrid_cov_err_over_bound", f"d{d}_tiles{-(-ld // 128)}", f"{np.nanmax(ec / bc):.3e} mean {np.nanmax(em / bm):.3e}")
    assert not bool((cb == TG.SENTINEL_BITS).any()) and not bool((mean_bits[:ld] == TG.SENTINEL_BITS).any()), "not written"
    assert bool((cov_bits[ld * ld:] == TG.SENTINEL_BITS).all()), "written past the ld x ld matrix"
    assert bool((mean_bits[ld:] == TG.SENTINEL_BITS).all()), "written past the ld means"
    assert torch.equal(cb, cb.T), "covariance not bitwise symmetric"
    assert (ec <= bc).all(), (d, float((ec / bc).max()), np.unravel_index(np.argmax(ec / bc), ec.shape))
    assert (em <= bm).all(), (d, float((em / bm).max()))
    # the zero columns d .. ld - 1 of the rows have zero mean and zero covariance with everything
    assert bool((cov[d:] == 0).all()) and bool((cov[:, d:] == 0).all()) and bool((mean[d:] == 0).all())
    # the prediction side against these statistics: the loss value (the gradient is tested where it is conditioned)
    my, Sy = LR.moment_stats(y)
    ref = float(np.abs(S64 - Sy).mean() + np.abs(m64 - my).mean())
    g = torch.zeros_like(by)
    loss = torch.zeros(4, device=DEV)
    ops.moment_fwd_bwd(mean.contiguous(), cov.contiguous(), by, n, d, 1.0, g, loss)
    torch.cuda.synchronize()
    got = float(loss[0])
    report("tilegrid_moment_loss", f"d{d}", f"{abs(got - ref) / max(1.0, abs(ref)):.3e}")
    assert abs(got - ref) < TG.MOMENT_TOL_LOSS * max(1.0, abs(ref)), (got, ref)
    assert bool(torch.isfinite(g).all()) and float(g[n:].abs().sum()) == 0.0 and float(g[:, d:].abs().sum()) == 0.0
