"""CPU checks of tests/_regime.py, which make tests/test_hip_regime.py meaningful: every generator has the properties its
text states, the "regime" loss cases are conditioned within the redraw cap, the float64 reference, the normalisers and the
float32 yardsticks agree with each other at the derived bounds, and the section-4 data is scale covariant bit for bit in
plain float32 arithmetic (so a GPU mismatch there belongs to the kernel)."""
import numpy as np
import pytest
import torch

import _loss_cases as LC
import _regime as RG
import _route_cases as RC
from _conv_ref import conv64, winograd_f32

U = 2.0 ** -24


def _live_rms_ratio(x, skip=()):
    rms = x[0].double().pow(2).mean(dim=(0, 1)).sqrt().numpy()
    live = rms > 0
    live[list(skip)] = False
    return rms[live].max() / rms[live].min()


# ------------------------------------------------------------------------------------------------------------ generators
@pytest.mark.parametrize("h,w,c", [(33, 20, 64), (43, 61, 256), (61, 67, 512)])
def test_activations_have_their_properties(h, w, c):
    x = RG.activations(h, w, c, 11)
    dead, single = RG.activation_info(h, w, c, 11)
    assert x.dtype == torch.float32 and tuple(x.shape) == (1, h, w, c) and bool((x >= 0).all()) and bool(torch.isfinite(x).all())
    assert torch.equal(x, RG.activations(h, w, c, 11)) and not torch.equal(x, RG.activations(h, w, c, 12))
    zero_ch = (x[0].amax(dim=(0, 1)) == 0).numpy()
    assert (zero_ch == dead).all() and 0.05 <= dead.mean() <= 0.15
    assert int((x[0, :, :, single] > 0).sum()) == 1
    share = (x[0] == 0).double().mean(dim=(0, 1)).numpy()
    others = ~dead
    others[single] = False
    assert (share[others] > 0.45).all() and (share[others] < 0.95).all()          # U[0.5, 0.9] per channel, sampled on h w pixels
    assert 0.6 <= float((x == 0).double().mean()) <= 0.9
    assert _live_rms_ratio(x, skip=[single]) >= 2.0 ** 10
    nz = x[0][:, :, others][x[0][:, :, others] > 0].double().log()
    gain_free = (x[0][:, :, others].double() / x[0][:, :, others].double().amax(dim=(0, 1))).flatten()
    assert float(nz.std()) > 1.0 and float(gain_free[gain_free > 0].median()) < 0.1      # heavy-tailed inside a channel


@pytest.mark.parametrize("h,w,c", [(10, 16, 512), (85, 128, 256), (170, 256, 128)])
def test_gradients_have_their_properties(h, w, c):
    g = RG.gradients(h, w, c, 5)
    assert g.dtype == torch.float32 and tuple(g.shape) == (1, h, w, c) and bool(torch.isfinite(g).all())
    support = int((g[0] != 0).any(dim=2).sum())
    assert support == min(RG.GRAD_PIXELS, h * w // 32) <= 4096
    nz = g[g != 0]
    assert 0.4 < float((nz > 0).double().mean()) < 0.6                            # signed
    assert 2.0 ** -29 < float(nz.abs().median()) < 2.0 ** -25                     # around 2^-27 (the gains are symmetric in log)
    assert float(nz.abs().min()) > 2.0 ** -60                                    # nowhere near the f32 subnormals
    assert _live_rms_ratio(g) >= 2.0 ** 10
    assert float((g == 0).double().mean()) >= 0.9


@pytest.mark.parametrize("cin,cout", [(64, 64), (256, 512)])
def test_weights_have_their_properties(cin, cout):
    w, b = RG.weights(cin, cout, 3)
    assert tuple(w.shape) == (3, 3, cin, cout) and tuple(b.shape) == (cout,)
    dead = RG.dead_outputs(cin, cout, 3)
    assert 0.05 <= dead.mean() <= 0.15 and (b[torch.from_numpy(dead)] == RG.DEAD_BIAS).all()
    live_b = b[torch.from_numpy(~dead)].double()
    assert 0.3 < float(live_b.std()) < 0.7 and abs(float(live_b.mean())) < 0.2
    he = (2.0 / (9 * cin)) ** 0.5
    out_rms = w.double().pow(2).mean(dim=(0, 1, 2)).sqrt() / he
    in_rms = w.double().pow(2).mean(dim=(0, 1, 3)).sqrt() / he
    assert float(out_rms.max() / out_rms.min()) >= 2.0 ** 4 and float(in_rms.max() / in_rms.min()) >= 2.0 ** 4
    # paired with regime activations, a live output still collects channel products spread over >= 2^10
    x = RG.activations(9, 9, cin, 3)
    per_ch = x[0].double().pow(2).mean(dim=(0, 1)).sqrt() * in_rms
    per_ch = per_ch[per_ch > 0]
    assert float(per_ch.max() / per_ch.min()) >= 2.0 ** 10


def test_a_dead_bias_kills_its_channel_on_regime_activations():
    for case in RG.CASES:
        if case[1] != "fwd":
            continue
        p = RG.Problem(case)
        worst = float(conv64(p.x.abs(), p.wt.abs()).max())
        assert worst < -RG.DEAD_BIAS / 4, (RC.case_id(case), worst)


def test_trunk_weights_on_the_golden_content_image():
    from oracle import strotss_oracle as O
    wts = RG.trunk_weights()
    ref = O.make_synthetic_vgg16_weights(0)
    assert len(wts) == len(ref) and all(a[0].shape == b[0].shape and a[1].shape == b[1].shape and a[0].dtype == torch.float32
                                        for a, b in zip(wts, ref))
    with torch.no_grad():
        taps = O.VGG(wts)(RG.golden_content_64())
    assert len(taps) == 9
    for t in taps:
        dead = float((t[0].amax(dim=(0, 1)) == 0).double().mean())
        assert dead >= 0.05, dead
        assert float((t == 0).double().mean()) >= 0.45
    p99 = [float(torch.quantile(t.flatten(), 0.99)) for t in taps]
    print("99th percentiles of the taps:", " ".join(f"{v:.1f}" for v in p99))
    assert 10.0 <= p99[-1] <= 1000.0 and p99[-1] > 5 * p99[0]                      # grows from block1 to block5


def test_loss_rows_have_their_properties():
    rng = np.random.default_rng(1)
    x, y = RG.loss_rows(rng, 400, 2179), RG.loss_rows(rng, 300, 2179)
    assert x.shape == (400, 2179) and (x >= 0).all() and (x[:, :3] <= 1).all() and np.isfinite(x).all()
    dead = x[:, 3:].max(0) == 0
    assert 0.05 <= dead.mean() <= 0.15 and ((y[:, 3:].max(0) == 0) == dead).all()          # the same columns in every call
    share = (x[:, 3:][:, ~dead] == 0).mean(0)
    assert (share > 0.5).all() and (share < 0.97).all() and 0.6 <= (x[:, 3:] == 0).mean() <= 0.9
    edges = np.cumsum((3,) + RG.TAP_CHANNELS)
    med = [np.median(b[b > 0]) for b in (x[:, lo:hi] for lo, hi in zip(edges[:-1], edges[1:]))]
    assert 0.5 < med[0] < 2.0 and 50.0 < med[-1] < 200.0 and all(b > a for a, b in zip(med, med[1:]))


@pytest.mark.parametrize("label", ["regime_n1000_ns777", "regime_small_n37"])
def test_regime_loss_cases_are_conditioned_within_the_cap(label):
    assert [c[1:] for c in LC.CASES if c[0] == label] == [{"regime_n1000_ns777": (1000, 777, 2179, "regime"),
                                                           "regime_small_n37": (37, 300, 2179, "regime")}[label]]
    c = LC.make_case(label)                          # raises after 50 redraws
    costs = LC.cost_matrices(c.x, c.y, c.d)
    for m in LC.METRICS:
        assert LC.conditioned(costs[m], c.gx, c.gy), m
    assert c.redrawn <= 50 * (c.n + c.ns)
    for v in (c.x, c.y, c.c):
        assert 0.6 <= (v[:, 3:] == 0).mean() <= 0.9 and 0.05 <= (v[:, 3:].max(0) == 0).mean() <= 0.15


# ------------------------------------------------------------------------------------------------------------ references
def test_cases_are_the_smallest_of_every_default_route():
    keys = {c[:2] for c in RC.DEFAULT_CASES}
    assert {c[:2] for c in RG.CASES} == keys and len(RG.CASES) == len(keys)
    assert {c[0] for c in RG.CASES} == set(RC.ROUTES)
    for c in RG.CASES:
        assert c in RC.DEFAULT_CASES
        assert all(c[2] * c[3] * c[4] * c[5] <= o[2] * o[3] * o[4] * o[5] for o in RC.DEFAULT_CASES if o[:2] == c[:2])
    assert not RC.misrouted(RG.CASES)


def _errors(p, tile):
    relu = p.direction == "fwd"
    ref = conv64(p.a, p.k) + (p.b.double() if p.b is not None else 0.0)
    ref = torch.relu(ref) if relu else ref
    norm = RG.normaliser(p.a, p.k, p.b, tile, conv64)
    got = RG.yardstick_f32(p.a, p.k, p.b, tile, relu)
    return ref, norm, got


@pytest.mark.parametrize("case", [c for c in RG.CASES if c[0].startswith("direct")], ids=RC.case_id)
def test_float32_direct_yardstick_is_within_the_derived_worst_case(case):
    """K = 9 cin products, each rounded once, summed in any order and added to the bias: every element of the float32 conv2d
    lies within K 2^-24 (|a| (*) |k| + |b|) of float64; an element whose normaliser is 0 is exactly 0."""
    p = RG.Problem(case)
    ref, norm, got = _errors(p, 0)
    e, zeros_ok = RG.element_error(got, ref, norm)
    K = 9 * p.a.shape[3]
    print(f"{RC.case_id(case)}: e_f32 = {e:.3e} = {e / U:.2f} u, bound {K} u; normaliser zero at "
          f"{float((norm == 0).double().mean()):.3f} of the elements")
    assert np.isfinite(e) and 0 < e < K * U and zeros_ok
    assert bool((ref.abs() <= norm * (1 + 1e-12)).all())                         # the normaliser bounds the reference


@pytest.mark.parametrize("tile,case", [(2, ("F2_gemm_f32", "fwd", 23, 29, 64, 64)), (2, ("F2_gemm_f32", "dgrad", 23, 29, 64, 64)),
                                        (4, ("F4_gemm_f32", "fwd", 43, 61, 64, 64)), (4, ("F4_gemm_f32", "dgrad", 43, 61, 64, 64))],
                         ids=["F2-fwd", "F2-dgrad", "F4-fwd", "F4-dgrad"])
def test_float32_winograd_yardstick_and_its_normaliser(tile, case):
    """The NumPy restatement is the convolution (float64 inputs of small integers: exact), its float32 error on regime data is
    finite and small against the window normaliser, and the normaliser is zero only where the whole window is."""
    g = torch.Generator().manual_seed(3)
    xi = torch.randint(-3, 4, (1, 13, 10, 8), generator=g).float()
    ki = torch.randint(-2, 3, (3, 3, 8, 5), generator=g).float() * 576.0
    assert torch.equal(winograd_f32(xi.numpy(), ki.numpy(), tile).double(), conv64(xi, ki))
    p = RG.Problem(case)
    ref, norm, got = _errors(p, tile)
    e, zeros_ok = RG.element_error(got, ref, norm)
    print(f"F({tile}x{tile}) {case[1]}: e_f32 = {e:.3e} = {e / U:.1f} u")
    assert np.isfinite(e) and 0 < e < 1e-3 and zeros_ok
    direct = RG.normaliser(p.a, p.k, p.b, 0, conv64)
    assert bool((norm >= direct * (1 - 1e-12)).all())                            # wider than the direct one, element by element
    if p.direction == "dgrad":
        assert 0.0 < float((norm == 0).double().mean()) < 1.0                    # sparse gradients: all-zero windows exist
        assert bool((ref[norm == 0] == 0).all())


# ------------------------------------------------------------------------------------------------------------ scale data
@pytest.mark.parametrize("case", RG.CASES, ids=RC.case_id)
def test_scale_data_is_covariant_in_plain_float32(case):
    """conv2d in float32 of the section-4 data scaled by 2^k equals 2^k times the unscaled result bit for bit, k = -40 and
    +40: no intermediate of plain f32 arithmetic underflows or overflows at these exponents."""
    d = RG.scale_problem(case)
    _, direction, h, w, cin, cout = case
    for v in (d["x"], d["gy"], d["b"]):
        assert torch.equal(v * 2.0 ** 20, torch.round(v * 2.0 ** 20))
    if direction == "fwd":
        a, k, b = d["x"], d["wt"].permute(3, 2, 0, 1).contiguous(), d["b"]
    else:
        a, k, b = d["gy"], d["wt"].flip(0, 1).permute(2, 3, 0, 1).contiguous(), None
    conv = lambda s: torch.nn.functional.conv2d((a * s).permute(0, 3, 1, 2), k, None if b is None else b * s, padding=1)
    base = conv(1.0)
    assert bool(torch.isfinite(base).all()) and float(base.abs().max()) > 0
    for e in RG.SCALE_EXPONENTS:
        s = 2.0 ** e
        assert torch.equal((a * s) / s, a)
        assert torch.equal(conv(s), base * s), e
