"""Capped launches past their caps on the MI355X ("Capped launches"): every `case` row of
tests/_launch_cap_cases.py at the smallest shape that asks for more workgroups than the launch has, so that the second trip of
the kernel's walk runs, element by element against the family's own float64 restatement within the family's own bound
(_smooth_ref, _upsample_ref, _pixel_ref, _color_ref, _exact_cases, _track_ref / _mask_edge_cases, _detail_map_ref), bit for
bit where the output is a copy, a code or a sign word.  Outputs are pre-filled (NaN, 255, all ones) where the operator takes
one; the bound is asserted over the whole output and over the walked region on its own, and the worst ratio of each is printed.
tests/test_launch_caps_cpu.py shows on the host that the same comparisons reject a walk that stops after its first trip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _launch_cap_cases as L  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
NAN = float("nan")


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _host(t):
    return t.detach().cpu().numpy()


def _settle(what, fig_bad):
    fig, bad = fig_bad
    print(f"MEASURE launch_caps {what}: " + ", ".join(f"{k} {v:.3f}" if isinstance(v, float) else f"{k} {v}" for k, v in fig.items()))
    assert not bad, (what, bad)


@pytest.mark.parametrize("hw,r", L.SMOOTH_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else f"r{v}")
def test_guided_smooth_past_both_tile_caps(hw, r):
    from nn import _ops
    h, w = hw
    assert L.smooth_cols_tiles(h, w) > L.D["SMOOTH_MAX_GRID"] and L.smooth_rows_tiles(h, w) > L.D["SMOOTH_MAX_GRID"]
    p, I = L.smooth_images(h, w, r)
    out = torch.full((h, w, 3), NAN, device=DEV)
    _ops.guided_smooth(_dev(p), _dev(I), r, L.SMOOTH_EPS, out=out)
    torch.cuda.synchronize()
    _settle(f"guided_smooth {h} x {w} r {r}", L.smooth_judge(h, w, r, _host(out)))
    if len(L.smooth_bands(h, w)) > 1:
        # between the float64 bands: every row is, bit for bit, what a launch BELOW both caps gives for it -- the image cut into
        # runs of rows with 2 r more on each side (the filter is local and its sums run in the same order wherever the rows lie)
        pd, Id, step, m = _dev(p), _dev(I), L.SMOOTH_CROP_ROWS, 2 * r
        for y0 in range(0, h, step):
            a, b = max(0, y0 - m), min(h, y0 + step + m)
            assert max(L.smooth_cols_tiles(b - a, w), L.smooth_rows_tiles(b - a, w)) <= L.D["SMOOTH_MAX_GRID"]
            crop = _ops.guided_smooth(pd[a:b].clone(), Id[a:b].clone(), r, L.SMOOTH_EPS)     # (a copy: 16-byte aligned)
            n = min(step, h - y0)
            differ = int((crop[y0 - a:y0 - a + n].view(torch.int32) != out[y0:y0 + n].view(torch.int32)).sum())
            assert differ == 0, (f"rows {y0}..{y0 + n}: {differ} elements differ from an unwalked launch's")


@pytest.mark.parametrize("r", L.UPS_RADII)
def test_guided_upsample_low_resolution_passes_past_both_tile_caps(r):
    from nn import _ops
    p, I_lo, I_hi = L.ups_inputs(r)
    pd, lod, hid = _dev(p), _dev(I_lo), _dev(I_hi)
    for mode in L.UPS_MODES:
        out = torch.full((*L.UPS_HI, 3), NAN, device=DEV)
        _ops.guided_upsample(pd, lod, hid, r, L.SMOOTH_EPS, mode, out=out)
        torch.cuda.synchronize()
        _settle(f"guided_upsample {L.UPS_LO} -> {L.UPS_HI} r {r} {mode}", L.ups_judge(r, mode, _host(out)))


@pytest.mark.parametrize("case", L.RESIZE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_past_32768_rows_of_workgroups(case):
    from nn import _ops
    ih, iw, oh, ow, c = case
    x, add = L.resize_data(case)
    for alpha, with_add in ((1.0, False), (-1.0, True)):
        out = torch.full((1, oh, ow, c), NAN, device=DEV)
        _ops.resize_bilinear(_dev(x)[None], oh, ow, alpha, _dev(add)[None] if with_add else None, out=out)
        torch.cuda.synchronize()
        _settle(f"resize {case} alpha {alpha}", L.resize_judge(case, alpha, with_add, _host(out)[0]))


@pytest.mark.parametrize("case", L.ADJOINT_CASES, ids=lambda c: "x".join(map(str, c)))
def test_resize_adjoint_past_32768_rows_of_workgroups(case):
    from nn import _ops
    ih, iw, oh, ow, c = case
    out = torch.full((1, ih, iw, c), NAN, device=DEV)
    _ops.resize_bilinear_adjoint(_dev(L.adjoint_data(case))[None], ih, iw, out=out)
    torch.cuda.synchronize()
    _settle(f"resize adjoint {case}", L.adjoint_judge(case, _host(out)[0]))


def test_maxpool_past_16384_rows_of_workgroups():
    """values, codes, the coded backward plain and accumulating against the restatement; the backward from the activations,
    plain and accumulating (a one-dimensional grid that is NOT past its 8192 workgroups at this shape: it is at 683 x 1024 x 64
    in test_hip_pixel_path.py, both forms), must give the bits of the coded one here too"""
    from nn import _ops
    h, w, c = L.POOL_TALL
    d = L.pool_data()
    xd, gd = _dev(d["x"])[None], _dev(d["gout"])[None]
    out = torch.full((1, h // 2, w // 2, c), NAN, device=DEV)
    code = torch.full((1, h // 2, w // 2, c), 255, dtype=torch.uint8, device=DEV)
    _ops.maxpool2_fwd(xd, out=out, code=code)
    gin = torch.full((1, h, w, c), NAN, device=DEV)
    _ops.maxpool2_bwd(xd, gd, out=gin, code=code)
    acc = _dev(d["base"])[None].clone()
    _ops.maxpool2_bwd(xd, gd, out=acc, code=code, accumulate=True)
    by_act = torch.full((1, h, w, c), NAN, device=DEV)
    _ops.maxpool2_bwd(xd, gd, out=by_act)
    acc_act = _dev(d["base"])[None].clone()
    _ops.maxpool2_bwd(xd, gd, out=acc_act, accumulate=True)
    torch.cuda.synchronize()
    _settle(f"maxpool {L.POOL_TALL}", L.pool_judge(dict(out=_host(out)[0], code=_host(code)[0], gin_code=_host(gin)[0],
                                                         acc_code=_host(acc)[0])))
    assert torch.equal(by_act.view(torch.int32), gin.view(torch.int32))
    assert torch.equal(acc_act.view(torch.int32), acc.view(torch.int32))


@pytest.mark.parametrize("kind", L.COLOR_WEIGHTS, ids=str)
def test_color_stats_past_2048_blocks(kind):
    from nn import _ops
    x, m = L.color_data(kind)
    got = _ops.color_stats(_dev(x), None if m is None else _dev(m))
    again = _ops.color_stats(_dev(x), None if m is None else _dev(m))
    torch.cuda.synchronize()
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))
    _settle(f"color_stats {L.COLOR_STATS_SHAPE} weight {kind}", L.color_judge(kind, _host(got)))


def test_relu_bits_past_8192_blocks():
    from nn import _ops
    h, w, c = L.RELU_BITS_SHAPE
    out = torch.full((L.cdiv(h, 4) * L.cdiv(w, 4), c), -1, dtype=torch.int32, device=DEV)
    _ops.relu_bits(_dev(L.relu_bits_data())[None], out=out)
    torch.cuda.synchronize()
    _settle(f"relu_bits {L.RELU_BITS_SHAPE}", L.relu_bits_judge(_host(out)))


@pytest.mark.parametrize("tile", L.WEIGHTS_TILES)
def test_winograd_weights_past_4096_blocks(tile):
    from nn import _ops
    u = _ops.winograd_weights(_dev(L.weights_data()), tile)
    torch.cuda.synchronize()
    _settle(f"winograd_weights {L.WEIGHTS_SHAPE} F{tile}", L.weights_judge(tile, _host(u)))


def test_assign_prior_past_2048_tiles():
    from nn import _ops
    n, d, k = L.ASSIGN_PRIOR_SHAPE
    (x, inv, c32, prior), _ = L.assign_want()
    got = _ops.kmeans_assign_prior(_dev(x), _dev(inv), n, d, _dev(c32), k, _dev(prior, torch.int32), L.ASSIGN_BETA)
    torch.cuda.synchronize()
    _settle(f"kmeans_assign_prior {L.ASSIGN_PRIOR_SHAPE}", L.assign_judge(tuple(_host(t) for t in got)))


def test_detail_map_past_its_three_caps():
    from nn import _ops
    h, w, r = L.DETAIL_SHAPE
    assert L.dm_cols_tiles(h, w) > L.D["DM_MAX_GRID"] and L.dm_rows_tiles(h, w) > L.D["DM_ROWS_MAX_GRID"]
    assert L.dm_scale_groups(h, w) > L.D["DM_SCALE_MAX_GRID"]
    img = L.detail_want()[0]
    got = _ops.detail_map(torch.from_numpy(np.ascontiguousarray(img)).cuda(), r, *L.DETAIL_PARAMS)
    torch.cuda.synchronize()
    assert got.dtype == torch.float32 and tuple(got.shape) == (h, w)
    _settle(f"detail_map {L.DETAIL_SHAPE}", L.detail_judge(_host(got)))


@pytest.mark.parametrize("group", sorted(L.CONV_GROUPS))
def test_winograd_transforms_past_16384_blocks(group):
    """one fresh child process per switch group, one at a time (tests/_launch_cap_conv_worker.py)"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_launch_cap_conv_worker.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    out = subprocess.run([sys.executable, worker, group], env=dict(env, **L.CONV_GROUPS[group]), capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    results = json.loads(out.stdout.strip().splitlines()[-1])
    assert sorted(results) == sorted(n for n, c in L.CONV_CASES.items() if c[0] == group)
    for name, (fig, bad) in results.items():
        _settle(f"{name} {L.CONV_CASES[name][2]} [{group}]", (fig, bad))


def _splitk_problem(direction, h, w, cin, cout):
    import _exact_cases as E
    import _route_cases as RC
    RC._model()
    p = E.make_int_problem(("direct_splitk", direction, h, w, cin, cout))
    p.a, p.k_eff = p.a.cuda(), p.k_eff.cuda()
    if p.bias is not None:
        p.bias = p.bias.cuda()
    fig = E.direct_conditions(p, extra=float(E.PRE_MAX) if direction == "dgrad" else 0.0)
    assert fig["sum"] < 1.0, fig
    return E, p


def test_splitk_finish_pool_past_64_blocks_a_row():
    """strotss_conv3x3_relu_pool_fwd on the exact family: activation, pooled copy and codes bit for bit"""
    from nn import _ops
    h, w, cin, cout = L.SPLITK_POOL_SHAPE
    assert _ops.conv3x3_direct_splits(h, w, cin, cout)
    E, p = _splitk_problem("fwd", h, w, cin, cout)
    pre = E.conv64(p.a, 576.0 * p.k_eff) + p.bias.double()
    E.assert_nontrivial(pre, "splitk pool")
    pool, code = E.pool_reference(pre)
    w_tok = p.wt.permute(0, 1, 3, 2).reshape(9, cout, cin).contiguous()
    out = torch.full((1, h, w, cout), NAN, device=DEV)
    pool_out = torch.full((1, h // 2, w // 2, cout), NAN, device=DEV)
    pool_code = torch.full((1, h // 2, w // 2, cout), 9, dtype=torch.uint8, device=DEV)
    _ops.conv3x3_relu_fwd(p.a, w_tok, p.bias, out=out, pool_out=pool_out, pool_code=pool_code)
    torch.cuda.synchronize()
    got = dict(out=_host(out)[0], pool=_host(pool_out)[0], code=_host(pool_code)[0])
    want = dict(out=torch.relu(pre)[0].float().cpu().numpy(), pool=pool[0].float().cpu().numpy(),
                code=code[0].to(torch.uint8).cpu().numpy())
    _settle(f"splitk finish pool {L.SPLITK_POOL_SHAPE}", L.splitk_pool_judge(got, want))


def test_splitk_finish_unpool_past_64_blocks_a_row():
    """strotss_conv3x3_dgrad_unpool on the exact family, plain and accumulating, bit for bit"""
    from nn import _ops
    H, W, cout, cin = L.SPLITK_UNPOOL_SHAPE
    h, w = H // 2, W // 2
    E, p = _splitk_problem("dgrad", h, w, cin, cout)
    conv = E.conv64(p.a, 576.0 * p.k_eff)
    E.assert_nontrivial(conv, "splitk unpool")
    w_tik = p.wt.flip(0, 1).reshape(9, cin, cout).contiguous()
    code = torch.randint(0, 5, (1, h, w, cin), generator=E._gen("caps:code"), dtype=torch.uint8).cuda()
    want = E.unpool_reference(conv, code)
    got = _ops.conv3x3_dgrad_unpool(p.a, w_tik, cin, code, torch.full((1, H, W, cin), NAN, device=DEV))
    base = torch.randint(-E.PRE_MAX, E.PRE_MAX + 1, (1, H, W, cin), generator=E._gen("caps:pre2")).float().cuda()
    acc = _ops.conv3x3_dgrad_unpool(p.a, w_tik, cin, code, base.clone(), accumulate=True)
    torch.cuda.synchronize()
    _settle(f"splitk finish unpool {L.SPLITK_UNPOOL_SHAPE}", L.splitk_unpool_judge(
        dict(gin=_host(got)[0], acc=_host(acc)[0]),
        dict(gin=want[0].float().cpu().numpy(), acc=(base.double() + want)[0].float().cpu().numpy())))


def test_x3_panel_split_past_2048_blocks():
    """strotss_conv3x3_winograd_x3pack on weights of 2^21 + 16384 values a position: the panels are the h, m, l planes of
    split3 in the layout of csrc/mfma_x3.h, bit for bit, over a pre-fill of bf16 NaN"""
    from nn import _hip, _ops
    rows, k = L.X3_SPLIT_SHAPE
    g = torch.Generator(device=DEV).manual_seed(rows + k)
    u = torch.randn((36, rows, k), generator=g, device=DEV) * torch.exp2(torch.randint(-12, 13, (36, rows, 1), generator=g, device=DEV).float())
    nb = int(_hip.lib().strotss_conv3x3_winograd_x3_bytes(rows, k))
    assert nb == 2 * 36 * 3 * rows * k
    up = torch.full((nb // 2,), NAN, dtype=torch.bfloat16, device=DEV)
    _ops.check(_hip.lib().strotss_conv3x3_winograd_x3pack(_ops.ptr(u), rows, k, _ops.ptr(up), _ops.stream_ptr()), "x3pack")
    torch.cuda.synchronize()
    want = L.x3_panels(u)
    assert bool((want[:, :, 1] != 0).any()) and bool((want[:, :, 2] != 0).any())          # the m and l planes are in use
    _settle(f"x3 panel split {L.X3_SPLIT_SHAPE}", L.x3_judge(_host(up.view(torch.int16)).reshape(want.shape),
                                                            _host(want.view(torch.int16))))


def test_sinkhorn_kernel_matrix_past_4096_blocks():
    """strotss_sinkhorn_cos_fwd_bwd at n ldm = 1025 x 1024: test_hip_sinkhorn.py's call and checks"""
    import _sinkhorn_ref as SR
    from _loss_harness import fbuf, run_entry
    from nn import _ops as ops
    c = L.sk_case()
    assert SR.conditioned(c, "cosine", L.SK_L)
    ref_l, ref_g = L.sk_want()
    bx, by = fbuf(c.x), fbuf(c.y)
    rs = ops.row_inv_norm(bx, c.ns)
    gs = 0.37
    got, loss, g0 = run_entry(ops, lambda gp, lo: ops.sinkhorn_cos_fwd_bwd(bx, rs, c.ns, by, c.n, c.d, L.SK_L, c.T, gs, gp, lo[0]),
                              c.n, c.d, np.abs(ref_g).max() * gs, 31)
    _settle(f"sinkhorn {L.SK_SHAPE}", L.sk_judge(float(loss[0, 0]), got / gs))
    _settle(f"sinkhorn {L.SK_SHAPE} zero base", L.sk_judge(float(loss[0, 0]), g0.astype(np.float64) / gs))


def test_center_kernel_past_2048_blocks():
    """the moment term's f32 GEMM form in a fresh child process (tests/_launch_cap_moment_worker.py)"""
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_launch_cap_moment_worker.py")
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    out = subprocess.run([sys.executable, worker], env=dict(env, **L.CENTER_ENV), capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    results = json.loads(out.stdout.strip().splitlines()[-1])
    for name in ("stats", "fwd_bwd"):
        _settle(f"center_kernel {L.CENTER_SHAPE} {name}", tuple(results[name]))
