"""GPU: every default convolution route on data shaped like a pretrained trunk's (tests/_regime.py), judged element by
element, and every deterministic route's covariance under a power-of-two scale, bit for bit.

Value regime.  The smallest DEFAULT_CASES entry of each (route, direction) runs through the entry points and weight layouts
of tests/test_hip_conv_routes.py check_case on regime data.  Each output element's error against the nine-GEMM float64
reference is divided by what that element sums (`_regime.normaliser`: |a| (*) |k| + |b| for the direct routes, the window
form for the Winograd ones); an element whose normaliser is 0 must be exactly 0.  The bound is no constant: the same
figure of a float32 CPU restatement of the route's algorithm on the same data (`_regime.yardstick_f32`), times 4 for a
different summation order over the same number of terms.  The max / max|ref| bound of test_hip_conv_routes.TOL holds too.
Every case prints both figures (REGIME lines); DESIGN.md section 6, "value regime", records them.

Scale covariance.  Scaling by 2^k commutes with every IEEE rounding while nothing underflows or overflows
(tests/test_regime_cpu.py shows that plain float32 arithmetic does neither on this data at k = -40, +40), so
fwd(2^k x, w, 2^k b) == 2^k fwd(x, w, b), dgrad(2^k gy) == 2^k dgrad(gy), winograd_weights(2^k g) == 2^k winograd_weights(g)
and the hypercolumn gather / sorted adjoint alike, compared with torch.equal after the exact rescale.  No convolution route
uses float atomics, so all of them are held to it; the atomic tap adjoint (hypercol_scatter) is left out, and so are the
cosine and L2 distance entries, which carry absolute clamps (1e-12 on a squared norm, 1e-6 on a squared distance) by
design and are therefore not scale covariant."""
import numpy as np
import pytest
import torch

import _regime as RG
import _route_cases as RC
from _conv_ref import conv64, sign_words
from test_hip_conv_routes import TOL, _err

pytestmark = pytest.mark.gpu

DEV = "cuda"
SLACK = 4.0            # a different summation order (MFMA trees, split-K) over the same number of terms


class Layer:
    """The entry points of one case, as check_case calls them: fwd(x, b, **kw) and dgrad(gy, **kw) on the case's route."""

    def __init__(self, case, wt):
        from nn import _ops as ops
        self.ops = ops
        route, direction, h, w, cin, cout = case
        M = RC._model()
        got = M.conv_route(h, w, cin, cout, dgrad=direction == "dgrad")
        assert got == route, (RC.case_id(case), "drifted to", got)
        self.tile = M.winograd_tile(h, w, cin, cout) if M.use_winograd(cin, cout) else 0
        assert self.tile == RG.tile_of(route), (route, self.tile)
        self.cin, self.cout = cin, cout
        wt = wt.to(DEV)
        if direction == "fwd":
            self.w = ops.winograd_weights(wt.permute(3, 2, 0, 1), self.tile) if self.tile else \
                wt.permute(0, 1, 3, 2).reshape(9, cout, cin).contiguous()
        else:
            self.w = ops.winograd_weights(wt.flip(0, 1).permute(2, 3, 0, 1), self.tile) if self.tile else \
                wt.flip(0, 1).reshape(9, cin, cout).contiguous()

    def fwd(self, x, b, **kw):
        return (self.ops.conv3x3_winograd_fwd if self.tile else self.ops.conv3x3_relu_fwd)(x, self.w, b, **kw)

    def dgrad(self, gy, **kw):
        return (self.ops.conv3x3_winograd_dgrad if self.tile else self.ops.conv3x3_dgrad)(gy, self.w, self.cin, **kw)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)          # an unwritten entry stays NaN and fails


def _judge(case, what, got, ref, norm, yard, results):
    """One quantity of one case: per-element error of the GPU and of the float32 yardstick, the same reference and normaliser."""
    route = case[0]
    e_gpu, zeros_gpu = RG.element_error(got, ref, norm)
    e_f32, zeros_f32 = RG.element_error(yard.to(DEV), ref, norm)
    mx = _err(got, ref)[0]
    tol = TOL.get(route, 5e-5)
    print(f"REGIME {RC.case_id(case):40s} {what:13s} e_gpu {e_gpu:.3e}  e_f32 {e_f32:.3e}  ratio {e_gpu / e_f32:.2f}  "
          f"max/max|ref| {mx:.2e} (tol {tol:.0e})  zero-normaliser share {float((norm == 0).double().mean()):.3f}")
    assert zeros_f32, "the yardstick is not 0 where the normaliser is"
    results.append((what, e_gpu, e_f32, zeros_gpu, mx, tol))


def _assert(case, results):
    for what, e_gpu, e_f32, zeros_gpu, mx, tol in results:
        assert np.isfinite(e_gpu) and e_f32 > 0
        assert zeros_gpu, (RC.case_id(case), what, "non-zero output where every term of the element is zero")
        assert e_gpu <= SLACK * e_f32, (RC.case_id(case), what, e_gpu, e_f32)
        assert mx < tol, (RC.case_id(case), what, mx, tol)


@pytest.mark.parametrize("case", RG.CASES, ids=RC.case_id)
def test_route_on_regime_data_per_element(case):
    route, direction, h, w, cin, cout = case
    p = RG.Problem(case)
    L = Layer(case, p.wt)
    ops, tile = L.ops, L.tile
    a, k = p.a.to(DEV), p.k.to(DEV)
    norm = RG.normaliser(a, k, None if p.b is None else p.b.to(DEV), tile, conv64)
    results = []
    if direction == "fwd":
        x, b = a, p.b.to(DEV)
        pre = conv64(x, k) + b.double()
        ref = torch.relu(pre)
        got = L.fwd(x, b, out=_nan(1, h, w, cout))
        _judge(case, "fwd", got, ref, norm, RG.yardstick_f32(p.a, p.k, p.b, tile, True), results)
        dead = torch.from_numpy(RG.dead_outputs(cin, cout, RG.case_seed(case))).to(DEV)
        assert bool(dead.any()) and bool((ref[..., dead] == 0).all()) and bool((got[..., dead] == 0).all()), "dead output channels"
        extra = {}
        if route != "direct":
            extra["pool_out"] = torch.full((1, h // 2, w // 2, cout), -1.0, device=DEV)
            extra["pool_code"] = torch.full((1, h // 2, w // 2, cout), 9, dtype=torch.uint8, device=DEV)
        if route.startswith("F4"):
            extra["relu_bits_out"] = ops.relu_bits_buffer(h, w, cout, DEV)
        if extra:
            got2 = L.fwd(x, b, out=torch.full_like(got, -7.0), **extra)
            assert torch.equal(got2, got), "the epilogue outputs change the activation"
        if "pool_out" in extra:
            code = torch.full_like(extra["pool_code"], 9)
            pooled = ops.maxpool2_fwd(got, code=code)
            win = got[0, :h // 2 * 2, :w // 2 * 2].reshape(h // 2, 2, w // 2, 2, cout)
            all_zero = (win.amax(dim=(1, 3)) == 0)
            assert 0.05 < float(all_zero.double().mean()) < 0.95, "the regime has all-zero pooling windows"
            assert torch.equal(extra["pool_out"], pooled), "pooled copy"
            assert torch.equal(extra["pool_code"], code), "argmax codes (the tie rule of all-zero windows included)"
            assert bool((code[0][all_zero] == code[0][all_zero][0]).all()), "one code for every all-zero window"
        if "relu_bits_out" in extra:
            words, valid = sign_words(got)
            bits = extra["relu_bits_out"].long() & 0xFFFFFFFF
            assert torch.equal(bits & valid, words), int(((bits & valid) != words).sum())
    else:
        gy, x = a, p.x.to(DEV)
        ref = conv64(gy, k)
        ref_masked = ref * (x > 0)
        yard = RG.yardstick_f32(p.a, p.k, None, tile, False)
        assert 0.0 < float((norm == 0).double().mean()) < 1.0, "the regime has windows without any gradient"
        _judge(case, "dgrad", L.dgrad(gy, out=_nan(1, h, w, cin)), ref, norm, yard, results)
        masked = L.dgrad(gy, act_in=x, out=_nan(1, h, w, cin))
        _judge(case, "dgrad_masked", masked, ref_masked, norm, yard * (p.x > 0), results)
        assert bool((masked[x == 0] == 0).all()), "masked entries"
        mask_kw = {"act_in": x}
        if route.startswith("F4"):
            xb = sign_words(x)[0].int()
            by_bits = L.dgrad(gy, relu_bits=xb, out=_nan(1, h, w, cin))
            assert torch.equal(by_bits, masked), "sign-word mask != activation mask"
            mask_kw["relu_bits"] = xb
        if route != "F2_gemm_f32":                  # (F(2x2,3x3) overwrites; the library refuses accumulate there)
            base = p.pre.to(DEV)                     # a base in the gradients' own regime: the sum is not absorbed by it
            acc = L.dgrad(gy, out=base.clone(), accumulate=True, **mask_kw)
            assert torch.equal(acc, base + masked), "accumulate != base + masked"
    _assert(case, results)


# ------------------------------------------------------------------------------------------------------------ scale
@pytest.mark.parametrize("case", RG.CASES, ids=RC.case_id)
def test_route_is_covariant_under_power_of_two_scales(case):
    route, direction, h, w, cin, cout = case
    d = {k: v.to(DEV) for k, v in RG.scale_problem(case).items()}
    L = Layer(case, d["wt"])
    ops = L.ops

    def run(s):
        out = {}
        if direction == "fwd":
            extra = {}
            if route != "direct":
                extra["pool_out"] = _nan(1, h // 2, w // 2, cout)
                extra["pool_code"] = torch.full((1, h // 2, w // 2, cout), 9, dtype=torch.uint8, device=DEV)
            if route.startswith("F4"):
                extra["relu_bits_out"] = ops.relu_bits_buffer(h, w, cout, DEV)
            out["fwd"] = L.fwd(d["x"] * s, d["b"] * s, out=_nan(1, h, w, cout), **extra)
            out.update(extra)
        else:
            out["dgrad"] = L.dgrad(d["gy"] * s, out=_nan(1, h, w, cin))
            out["dgrad_masked"] = L.dgrad(d["gy"] * s, act_in=d["x"], out=_nan(1, h, w, cin))
        return out

    base = run(1.0)
    for v in base.values():
        assert v.dtype != torch.float32 or bool(torch.isfinite(v).all())
    assert float(base["fwd" if direction == "fwd" else "dgrad"].abs().max()) > 0
    for e in RG.SCALE_EXPONENTS:
        s = 2.0 ** e
        for name, v in run(s).items():
            if name == "relu_bits_out":
                valid = sign_words(base["fwd"])[1]
                assert torch.equal(v.long() & valid, base[name].long() & valid), (RC.case_id(case), name, e)
                continue
            want = base[name] * s if v.dtype == torch.float32 else base[name]
            bad = int((v != want).sum())
            assert torch.equal(v, want), (RC.case_id(case), name, f"2^{e}", f"{bad} of {v.numel()} elements differ")


@pytest.mark.parametrize("tile", [2, 4])
def test_winograd_weights_are_covariant_under_power_of_two_scales(tile):
    """zeros included: taps that cancel exactly in G g G^T (equal taps in a column, a lone centre tap, an all-zero kernel)
    must stay exact zeros at every scale, which the kernel decides on `un == 0.0`"""
    from nn import _ops as ops
    g = torch.Generator().manual_seed(17)
    k = torch.round(torch.randn(64, 64, 3, 3, generator=g) * (2.0 / (9 * 64)) ** 0.5 * 2.0 ** 20) / 2.0 ** 20
    k[0] = 0.0
    k[1, :, :, :] = k[1, :, :1, :1]                    # nine equal taps: rows of G that sum to 0 cancel
    k[2] = 0.0
    k[2, :, 1, 1] = 0.5                                # a lone centre tap
    k[3, :, 2, :] = -k[3, :, 0, :]                     # antisymmetric in r
    k = k.to(DEV)
    base = ops.winograd_weights(k, tile)
    assert 0.0 < float((base == 0).double().mean()) < 0.5 and bool((base[:, 0] == 0).all())
    for e in RG.SCALE_EXPONENTS:
        got = ops.winograd_weights(k * 2.0 ** e, tile)
        assert torch.equal(got, base * 2.0 ** e), (tile, e, int((got != base * 2.0 ** e).sum()))
        assert torch.equal(got == 0, base == 0)


def test_hypercolumn_gather_and_sorted_adjoint_are_covariant_under_power_of_two_scales():
    """one small map set (a 32 x 48 image and its nine taps), 300 bilinear samples (fractional on the pooled maps); the atomic adjoint is not held to it"""
    from nn import _hip, _ops as ops
    from oracle import strotss_oracle as O
    h, w, n = 32, 48, 300
    g = torch.Generator().manual_seed(23)
    q = lambda t: torch.round(t * 2.0 ** 20) / 2.0 ** 20
    shapes = [(h, w, 3), (h, w, 64), (h, w, 64), (h // 2, w // 2, 128), (h // 2, w // 2, 128), (h // 4, w // 4, 256),
              (h // 4, w // 4, 256), (h // 4, w // 4, 256), (h // 8, w // 8, 512), (h // 16, w // 16, 512)]
    maps = [q(torch.relu(torch.randn(1, *s, generator=g))).to(DEV) for s in shapes]
    idx = torch.from_numpy(O.make_indices(h, w, True, n, np.random.default_rng(3))).to(DEV)
    d = sum(s[2] for s in shapes)
    gfeat = torch.zeros(ops.pad32(n), ops.pad32(d), device=DEV)
    gfeat[:n, :d] = q(torch.randn(n, d, generator=g)).to(DEV)
    divs = ops.map_divisors([s[:2] for s in shapes])

    def run(s):
        feats = ops.hypercol_gather([m * s for m in maps], idx, True)
        gm = [torch.zeros_like(m) for m in maps]
        mt = _hip.make_maps(maps, divs, gm)
        plan = ops.hypercol_scatter_plan(mt, idx)
        ops.hypercol_scatter_sorted(mt, plan, n, gfeat * s, relu_mask_from=1)
        torch.cuda.synchronize()
        return feats, gm

    f0, g0 = run(1.0)
    assert float(f0.abs().max()) > 0 and all(float(m.abs().max()) > 0 for m in g0)
    for e in RG.SCALE_EXPONENTS:
        s = 2.0 ** e
        f, gm = run(s)
        assert torch.equal(f, f0 * s), ("gather", e)
        for k, (a, b) in enumerate(zip(gm, g0)):
            assert torch.equal(a, b * s), ("sorted adjoint", k, e)
