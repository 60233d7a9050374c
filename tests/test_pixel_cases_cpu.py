"""CPU side of the pixel-path tests: the float64 references of tests/_pixel_ref.py against oracle/strotss_oracle.py, the property
every case of tests/_pixel_cases.py was built for, the footprints of the fused fold and fold adjoint at every size the GPU file
launches, and -- for every bound -- an error of the kind the bound exists for, planted into a copy of the reference's output and
rejected by the same check the GPU file uses."""
import numpy as np
import pytest
import torch

import _pixel_cases as PC
import _pixel_ref as R
from oracle import strotss_oracle as O

U = R.U


def f32(x):
    return np.asarray(x, np.float64).astype(np.float32)


# ------------------------------------------------------------------ references against the oracle
@pytest.mark.parametrize("case", PC.RESIZE_RATIOS + [(42, 64, 85, 128, 3), (85, 128, 42, 64, 3), (5, 1, 2, 1, 3)])
def test_resize_reference_is_the_oracle_and_the_dense_matrices(case):
    ih, iw, oh, ow, c = case
    if ih * iw > 400 * 600:
        ih, iw = ih // 4, iw // 4                      # the same ratio class, small enough for the dense matrices
    x = PC.image(ih, iw, c=c)
    ref, s = R.resize(x, oh, ow)
    orc = O.resize_bilinear(torch.from_numpy(x).double(), oh, ow).numpy()
    assert np.abs(ref - orc).max() <= 1e-12
    ay, ax = R.axis_matrix(ih, oh), R.axis_matrix(iw, ow)
    dense = np.einsum("ojc,pj->opc", np.einsum("oi,ijc->ojc", ay, x.astype(np.float64)), ax)
    assert np.abs(ref - dense).max() <= 1e-12
    assert np.allclose(ay.sum(1), 1, atol=1e-15) and np.allclose(ax.sum(1), 1, atol=1e-15)
    assert (s >= np.abs(ref) - 1e-12).all()            # the plain sum dominates the interpolated value
    # the float32 evaluation of the oracle's own formula meets the bound (the bound is not vacuous and not too tight)
    got = O.resize_bilinear(torch.from_numpy(x), oh, ow).numpy()
    assert R.check(got, ref, R.resize_bound(s), "float32 oracle") <= 1.0


@pytest.mark.parametrize("case", [(42, 64, 85, 128, 3), (21, 32, 42, 64, 1), (80, 120, 10, 16, 3), (5, 7, 60, 90, 8), (1, 1, 4, 3, 3),
                                  (7, 5, 1, 1, 3), (5, 1, 2, 1, 3)])
def test_adjoint_reference_is_the_transposed_matrices_and_the_oracles_gradient(case):
    ih, iw, oh, ow, c = case
    g = PC.normal((oh, ow, c), "adj", *case)
    ref, b, m = R.adjoint(g, ih, iw)
    ay, ax = R.axis_matrix(ih, oh), R.axis_matrix(iw, ow)
    dense = np.einsum("ipc,pj->ijc", np.einsum("oi,opc->ipc", ay, g.astype(np.float64)), ax)
    assert np.abs(ref - dense).max() <= 1e-12
    assert np.abs(b - np.einsum("ipc,pj->ijc", np.einsum("oi,opc->ipc", ay, np.abs(g).astype(np.float64)), ax)).max() <= 1e-12
    assert np.array_equal(m[:, :, 0], np.outer((ay != 0).sum(0), (ax != 0).sum(0)))
    x = torch.zeros(ih, iw, c, dtype=torch.float64, requires_grad=True)
    (O.resize_bilinear(x, oh, ow) * torch.from_numpy(g).double()).sum().backward()
    assert np.abs(ref - x.grad.numpy()).max() <= 1e-12
    if ih > 4 * oh:
        assert (m == 0).any() and (ref[(m == 0)[:, :, 0]] == 0).all()      # strong downscale: pixels without a contributing output


def test_first_layer_reference_is_the_oracles_vgg():
    w, b = R.first_layer_weights()
    for h, wd in [(17, 129), (42, 64)]:
        img = PC.image(h, wd)
        pre, bound = R.first_layer(img, w, b)
        vgg = O.VGG(O.make_synthetic_vgg16_weights(0), taps=("block1_conv1",))
        orc = vgg(torch.from_numpy(img)[None])[0][0].numpy()
        # the oracle divides by the float64 std, the reference multiplies by fl32(1 / std) as the kernel does: 2u of every term
        assert (np.abs(np.maximum(pre, 0) - orc) <= 3 * U * bound / (R.FIRST_LAYER_K * U)).all()
        assert np.array_equal(R.first_layer(img, w, b, rows=(3, 9))[0], pre[3:9])
        # data-gradient: <conv(p), g> differentiated
        g = PC.normal((h, wd, 64), "dg", h, wd)
        ref, bb = R.first_layer_dgrad(g, w)
        x = torch.from_numpy(img).double().requires_grad_(True)
        mean, istd = R.preprocess_constants()
        p = (x - torch.from_numpy(mean).double()) * torch.from_numpy(istd).double()
        y = torch.nn.functional.conv2d(p.permute(2, 0, 1)[None], torch.from_numpy(w).double().reshape(3, 3, 3, 64).permute(3, 2, 0, 1),
                                       padding=1)[0].permute(1, 2, 0)
        assert np.abs(y.detach().numpy() + b.astype(np.float64) - pre).max() <= 1e-12
        (y * torch.from_numpy(g).double()).sum().backward()
        assert np.abs(ref - x.grad.numpy()).max() <= 1e-11
        assert (bb >= np.abs(ref) - 1e-12).all()


@pytest.mark.parametrize("hw", [hw for hw in PC.FIRST_LAYER_SIZES if hw[0] * hw[1] <= 341 * 512])
@pytest.mark.parametrize("law", ["uniform", "blocks"])
def test_few_first_layer_signs_are_undecided(hw, law):
    """the sign words are compared with the float64 sign wherever |pre-activation| exceeds the element's bound: the elements
    left out must be at most 1e-3 of all, by the reference alone"""
    w, b = R.first_layer_weights()
    pre, bound = R.first_layer(PC.image(*hw, law=law), w, b)
    assert (np.abs(pre) <= bound).mean() <= 1e-3
    if law == "blocks":
        img = PC.image(*hw, law=law)
        assert (img == 0).any() and (img == 1).any()


@pytest.mark.parametrize("hwc", [s for s in PC.POOL_SHAPES if s[0] * s[1] * s[2] <= 170 * 256 * 256])
def test_pool_cases_and_reference(hwc):
    h, w, c = hwc
    x = PC.pool_input(h, w, c)
    v = R.windows(x)
    mx, code = R.maxpool(x)
    orc = torch.nn.functional.max_pool2d(torch.from_numpy(x).permute(2, 0, 1)[None], 2, 2)[0].permute(1, 2, 0).numpy()
    assert np.array_equal(mx, orc)
    if h * w >= 7 * 6 * 4 * 4:
        for a in range(4):
            for b in range(a + 1, 4):
                tie = (v[a] == mx) & (v[b] == mx) & (mx > 0)
                assert tie.any(), (a, b)                                  # a positive tie in every pair of window positions ...
                assert (code[tie] <= a).all()                             # ... resolved to the first in scan order
        assert (mx == 0).all(axis=2).any() and (code[mx == 0] == 4).all()  # all-zero windows: no gradient
    gout = PC.normal(mx.shape, "poolg", h, w, c)
    gin = R.maxpool_bwd(code, gout, h, w)
    assert np.isclose(gin.astype(np.float64).sum(), gout[code < 4].astype(np.float64).sum())
    base = PC.pool_base(h, w, c)
    assert not (base == 0).any() and np.array_equal((base + np.float32(0)).view(np.uint32), base.view(np.uint32))


def test_rmsprop_reference_and_gradient_law():
    lr, rho, eps = (float(np.float32(v)) for v in (PC.LR, PC.RHO, PC.EPS))
    assert np.float32(1.0) - np.float32(PC.RHO) == 1.0 - rho             # 1 - rho is exact in float32
    n = 4096
    var, rms = PC.normal((n,), "v").astype(np.float64), np.zeros(n)
    v_t, r_t = torch.from_numpy(var.copy()), torch.from_numpy(rms.copy())
    for step in range(PC.RMSPROP_STEPS):
        g = PC.rmsprop_gradient(n, step, 0)
        assert (g == 0).mean() > 1 / 32 and np.abs(g[g != 0]).min() >= 0.99e-12 and np.abs(g).max() <= 1.01e3
        assert (g[g != 0].astype(np.float32) ** 2 >= np.finfo(np.float32).tiny).all()
        rms, _, var, _ = R.rmsprop(var, rms, g, PC.LR, PC.RHO, PC.EPS)
        O.rmsprop_update(v_t, r_t, torch.from_numpy(g).double(), lr, rho, eps)
        assert np.allclose(rms, r_t.numpy(), rtol=1e-14, atol=0) and np.allclose(var, v_t.numpy(), rtol=1e-13, atol=1e-300)
        if step == 0:
            assert (var[g == 0] == PC.normal((n,), "v").astype(np.float64)[g == 0]).all()     # 0 / (0 + eps) moves nothing
    assert all(len(v) <= 8 for v in PC.RMSPROP_SETS.values()) and len(PC.RMSPROP_SETS["unequal"]) == 8
    assert all(max(v) > 2048 * 256 for v in PC.RMSPROP_SETS.values()) and 1 in PC.RMSPROP_SETS["unequal"]   # the capped grid loops


@pytest.mark.parametrize("plant", PC.POSTPROCESS_PLANTS)
@pytest.mark.parametrize("law", PC.POSTPROCESS_LAWS)
def test_postprocess_cases(law, plant):
    n = PC.POSTPROCESS_LENGTHS[2]
    assert n % 256 and PC.POSTPROCESS_LENGTHS[0] % 256 == 0
    lo_first, hi_first = PC.postprocess_input(n, law, plant)
    for x, planted_is_min in ((lo_first, True), (hi_first, False)):
        c = np.clip(x, 0, 1)
        assert c.max() > c.min()
        where = int(np.argmin(x) if planted_is_min else np.argmax(x))
        if plant == "first":
            assert where == 0
        if plant == "last":
            assert where == n - 1
        if plant == "tail":
            assert where >= n // 256 * 256
        if plant == "strided":
            assert 1024 * 256 <= where < n // 256 * 256
        if law != "outside":
            assert (c == c[where]).sum() == 1                      # only the planted element holds the extreme
        if law == "integers":
            assert c.min() == 0 and c.max() == 1
            assert (np.floor(c * np.float32(255)) == c * np.float32(255)).mean() > 0.2
    assert law != "outside" or ((lo_first < 0).any() and (lo_first > 1).any())


# ------------------------------------------------------------------ the fused forms' footprints, before anything is launched
def _all_pyramids():
    return [PC.chain(h, w) for h, w in PC.IMAGE_SIZES + PC.SEGMENT_EDGES + PC.sweep_sizes()]


def test_footprints_fit_the_lds_regions_wherever_the_host_admits():
    """fold: from a 32-pixel tile the footprint [tap(lo).lo, tap(hi).hi] of every level stays within 24; adjoint pairs: the
    middle-level region (own 16-pixel tile joined with what the 8-pixel tile gathers from) within 32, by the true contributors
    and by the kernel's widest candidate window.  Every halving pyramid is admitted by the fold's rule and walks in pairs."""
    worst_fold, worst_true, worst_window = 0, 0, 0
    for sizes in _all_pyramids():
        assert R.host_admits_fold(sizes), sizes
        assert [n for _, n in R.adjoint_groups(sizes)] == [2, 2, 1], sizes
        for ax in (0, 1):
            ns = tuple(hw[ax] for hw in sizes)
            worst_fold = max(worst_fold, max(R.fold_footprint_sides(ns)))
            for k in (0, 2):
                t, wn = R.adjoint_pair_region_sides(*ns[k:k + 3])
                assert t <= wn
                worst_true, worst_window = max(worst_true, t), max(worst_window, wn)
        assert R.fused_forms_fit(sizes)
    print(f"MEASURE pixel footprint fold {worst_fold} of {R.FOLD_REGION}, adjoint pair {worst_true} (true) {worst_window} (window) "
          f"of {R.ADJ2_REGION}")
    assert worst_fold <= R.FOLD_REGION and worst_window <= R.ADJ2_REGION
    for sizes in PC.REFUSED_PYRAMIDS:
        assert not R.host_admits_fold(sizes)


def test_candidate_windows_hold_every_contributor():
    """the adjoint kernels look for contributing outputs in a float32 window 'with a +-1 safety margin': at every (input,
    output) length pair of the sweep's chains, of the schedule and of the ratio cases, under either rounding of the window
    formula, the window holds every output whose tap table names the input pixel"""
    pairs = set()
    for sizes in _all_pyramids():
        for a, b in zip(sizes[:-1], sizes[1:]):
            pairs.update({(b[0], a[0]), (b[1], a[1]), (a[0], b[0]), (a[1], b[1])})
    for ih, iw, oh, ow, _ in PC.ADJOINT_RATIOS:
        pairs.update({(ih, oh), (iw, ow)})
    for n_in, n_out in sorted(pairs):
        first, last = R.contributors(n_in, n_out)
        (o0, o1), (w0, w1) = R.candidate_window(n_in, n_out)
        has = first <= last
        assert (o0[has] <= first[has]).all() and (o1[has] >= last[has]).all(), (n_in, n_out)
        assert (w0 <= o0).all() and (w1 >= o1).all()


# ------------------------------------------------------------------ the checks can fail
def test_planted_first_layer_column_shift_is_rejected():
    """the pixel column x = 128 (the first of a second segment) computed from the patch one pixel to the left"""
    w, b = R.first_layer_weights()
    img = PC.image(17, 257)
    pre, bound = R.first_layer(img, w, b)
    ref = np.maximum(pre, 0)
    assert R.check(f32(ref), ref, bound, "clean") <= 1.0
    bad = ref.copy()
    bad[:, 128] = ref[:, 127]
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), ref, bound, "shifted column")
    err = np.abs(bad - ref)[:, 128]
    assert np.median(err[err > 0] / bound[:, 128][err > 0]) > 1e3


def test_planted_dropped_dgrad_tap_is_rejected():
    """one of the nine taps dropped along one tile edge (row 4 of a 4 x 32 tiling takes no tap from row 3)"""
    w, _ = R.first_layer_weights()
    h, wd = 17, 129
    g = PC.normal((h, wd, 64), "dg", h, wd)
    ref, b = R.first_layer_dgrad(g, w)
    bound = R.DGRAD_K * U * b
    assert R.check(f32(ref), ref, bound, "clean") <= 1.0
    g2 = np.zeros((h + 2, wd + 2, 64)); g2[1:-1, 1:-1] = g
    _, istd = R.preprocess_constants()
    w4 = w.astype(np.float64).reshape(3, 3, 3, 64)
    bad = ref.copy()
    # pixel (4, x) takes gout[3, x] through dy = 2, dx = 1
    bad[4] -= (g2[4, 1:-1] @ w4[2, 1].T) * istd.astype(np.float64)
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), ref, bound, "dropped tap")
    assert np.median(np.abs(bad - ref)[4] / bound[4]) > 50


def test_planted_missing_adjoint_row_is_rejected():
    """one candidate output row missing from the window of one input row"""
    ih, iw, oh, ow = 42, 64, 85, 128
    g = PC.normal((oh, ow, 3), "adj", ih, iw)
    ref, b, m = R.adjoint(g, ih, iw)
    bound = R.adjoint_bound(b, m)
    assert R.check(f32(ref), ref, bound, "clean") <= 1.0
    first, last = R.contributors(ih, oh)
    g_cut = g.copy()
    g_cut[last[20]] = 0                                   # input row 20 (and its neighbour) never sees its last output row
    bad = ref.copy()
    bad[20] = R.adjoint(g_cut, ih, iw)[0][20]
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), ref, bound, "missing row")
    assert np.median(np.abs(bad - ref)[20] / bound[20]) > 1e3
    # an unwritten element and a -0.0 where nothing contributes
    assert not R.plus_zero(np.float32([0.0, -0.0])) and R.plus_zero(np.float32([0.0, 0.0]))
    nan = f32(ref); nan[3, 5, 1] = np.nan
    with pytest.raises(AssertionError, match="not finite"):
        R.check(nan, ref, bound, "sentinel")


def test_planted_resize_neighbour_tap_is_rejected():
    """one output column interpolated from taps one pixel off, and a lerp weight with a float32 rounding error of its own"""
    x = PC.image(42, 64)
    ref, s = R.resize(x, 85, 128)
    bound = R.resize_bound(s)
    assert R.check(f32(ref), ref, bound, "clean") <= 1.0
    bad = ref.copy(); bad[:, 77] = ref[:, 78]
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), ref, bound, "neighbour")
    bad = ref * (1 + 40 * U)
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), ref, bound, "40 u")


def test_planted_last_maximum_code_is_rejected():
    x = PC.pool_input(20, 28, 8)
    v = R.windows(x)
    mx, code = R.maxpool(x)
    last = np.where(mx > 0, 3 - np.argmax(v[::-1], axis=0), 4).astype(np.uint8)
    assert not np.array_equal(last, code) and (last >= code).all()
    assert np.array_equal(v.max(0), mx)                                   # the values alone do not notice ...
    gout = PC.normal(mx.shape, "poolg", 20, 28, 8)
    assert not np.array_equal(R.maxpool_bwd(last, gout, 20, 28), R.maxpool_bwd(code, gout, 20, 28))   # ... the codes and the backward do


def test_planted_float64_rho_is_rejected():
    n = 1 << 16
    g = PC.rmsprop_gradient(n, 1, 0)
    rms0 = (PC.rmsprop_gradient(n, 0, 0).astype(np.float64) ** 2 * 0.01).astype(np.float32)
    var0 = PC.normal((n,), "v")
    r, rb, v, vb = R.rmsprop(var0, rms0, g, PC.LR, PC.RHO, PC.EPS)
    assert R.check(f32(r), r, rb, "clean rms") <= 1.0 and R.check(f32(v), v, vb, "clean var") <= 1.0
    bad = 0.99 * rms0.astype(np.float64) + (1 - 0.99) * g.astype(np.float64) ** 2        # rho = 0.99, not fl32(0.99)
    with pytest.raises(AssertionError, match="over their bound"):
        R.check(f32(bad), r, rb, "float64 rho")
    assert abs(float(np.float32(0.99)) - 0.99) / 0.01 > 5 * 3 * U          # the (1 - rho) g g term moves by 16u: five bounds


def test_planted_minimum_missed_in_the_tail_is_rejected():
    n = PC.POSTPROCESS_LENGTHS[2]
    x = PC.postprocess_input(n, "inside", "tail")[0]
    ref = O.postprocess(torch.from_numpy(x)[None])
    f = np.clip(x, 0, 1)
    mn = f[:n // 256 * 256].min()                                          # a reduction that stops at the last full 256
    bad = (((f - mn) / (f - mn).max()) * np.float32(255)).astype(np.uint8)
    assert mn > f.min() and (bad != ref).mean() > 0.5
    same = (((f - f.min()) / (f - f.min()).max()) * np.float32(255)).astype(np.uint8)
    assert np.array_equal(same, ref)
