"""GPU: every convolution route the product runs (tests/_route_cases.py) against a float64 reference of the same layer.

Each case first asserts that the policy still sends its layer and direction to the labelled route (a drifted case fails,
it does not skip), then runs the layer through the same entry point and weights the trunk uses (nn/model.py) and compares
it with nine shifted float64 GEMMs (torch.matmul, none of the project's kernels; checked against
torch.nn.functional.conv2d below).  Forward: bias + ReLU, the pooled copy and its argmax codes, the sign words where the
route writes them.  Data-gradient: plain, masked by the input activation, masked by its sign words, and accumulating.
Tolerances are DESIGN.md 6's: the max abs error relative to max|ref| stays below 3e-6 (direct), 1e-5 (F(2x2,3x3)),
5e-5 (F(4x4,3x3), f32 or bf16x3 GEMMs).  The switch groups run in a child process (the library reads them once)."""
import json
import os
import subprocess
import sys
import zlib

import pytest
import torch

import _route_cases as RC
from _conv_ref import conv64 as _conv64, sign_words as _sign_words

pytestmark = pytest.mark.gpu

TOL = {"direct": 3e-6, "direct_splitk": 3e-6, "F2_gemm_f32": 1e-5}      # every F(4x4,3x3) route: 5e-5


def _err(got, ref):
    m = float(ref.abs().max()) or 1e-30
    e = (got.double() - ref).abs()
    return float(e.max()) / m, float(e.pow(2).mean().sqrt()) / m


def check_case(case):
    """Runs one case; returns {quantity: (max, rms) error relative to max|ref|}.  Raises on a failed check."""
    route, direction, h, w, cin, cout = case
    M = RC._model()
    from nn import _ops as ops
    assert M.conv_route(h, w, cin, cout, dgrad=direction == "dgrad") == route, (RC.case_id(case), "drifted to",
                                                                                M.conv_route(h, w, cin, cout, dgrad=direction == "dgrad"))
    tol = TOL.get(route, 5e-5)
    g = torch.Generator(device="cuda").manual_seed(zlib.crc32(RC.case_id(case).encode()))
    x = torch.relu(torch.randn(1, h, w, cin, generator=g, device="cuda"))
    wt = torch.randn(3, 3, cin, cout, generator=g, device="cuda") * (2.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g, device="cuda") * 0.1
    tile = M.winograd_tile(h, w, cin, cout) if M.use_winograd(cin, cout) else 0      # the trunk's per-layer decision
    assert (tile == 0) == route.startswith("direct") and (tile == 2) == (route == "F2_gemm_f32"), (route, tile)
    res = {}
    if direction == "fwd":
        if tile:
            u = ops.winograd_weights(wt.permute(3, 2, 0, 1), tile)
            fwd = lambda **kw: ops.conv3x3_winograd_fwd(x, u, b, **kw)
        else:
            w_tok = wt.permute(0, 1, 3, 2).reshape(9, cout, cin).contiguous()
            fwd = lambda **kw: ops.conv3x3_relu_fwd(x, w_tok, b, **kw)
        ref = torch.relu(_conv64(x, wt) + b.double())
        got = fwd(out=torch.full((1, h, w, cout), float("nan"), device="cuda"))      # an unwritten entry stays NaN and fails
        res["fwd"] = _err(got, ref)
        extra = {}
        if route != "direct":                 # (the one-pass direct kernel has no pooling epilogue)
            extra["pool_out"] = torch.full((1, h // 2, w // 2, cout), -1.0, device="cuda")
            extra["pool_code"] = torch.full((1, h // 2, w // 2, cout), 9, dtype=torch.uint8, device="cuda")
        if route.startswith("F4"):
            extra["relu_bits_out"] = ops.relu_bits_buffer(h, w, cout, "cuda")
        if extra:                             # the trunk's call: everything the epilogue writes at once
            got2 = fwd(out=torch.full_like(got, -7.0), **extra)
            assert torch.equal(got2, got), "the epilogue outputs change the activation"
        if "pool_out" in extra:
            want = torch.nn.functional.max_pool2d(got.permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
            assert torch.equal(extra["pool_out"], want), "pooled copy"
            code = torch.empty_like(extra["pool_code"])
            ops.maxpool2_fwd(got, code=code)
            assert torch.equal(extra["pool_code"], code), "argmax codes"
        if "relu_bits_out" in extra:
            words, valid = _sign_words(got)
            bits = extra["relu_bits_out"].long() & 0xFFFFFFFF
            assert torch.equal(bits & valid, words), int(((bits & valid) != words).sum())
    else:
        if tile:
            u = ops.winograd_weights(wt.flip(0, 1).permute(2, 3, 0, 1), tile)
            dg = lambda **kw: ops.conv3x3_winograd_dgrad(gy, u, cin, **kw)
        else:
            w_tik = wt.flip(0, 1).reshape(9, cin, cout).contiguous()
            dg = lambda **kw: ops.conv3x3_dgrad(gy, w_tik, cin, **kw)
        gy = torch.randn(1, h, w, cout, generator=g, device="cuda")
        ref = _conv64(gy, wt.flip(0, 1).transpose(2, 3))
        ref_masked = ref * (x > 0)
        nan = lambda: torch.full((1, h, w, cin), float("nan"), device="cuda")       # an unwritten entry stays NaN and fails
        res["dgrad"] = _err(dg(out=nan()), ref)
        masked = dg(act_in=x, out=nan())
        res["dgrad_masked"] = _err(masked, ref_masked)
        mask_kw = {"act_in": x}
        if route.startswith("F4"):            # the mask from the input's sign words: the same bits, the same result
            xb = _sign_words(x)[0].int()
            by_bits = dg(relu_bits=xb, out=nan())
            res["dgrad_bits"] = _err(by_bits, ref_masked)
            assert torch.equal(by_bits, masked), "sign-word mask != activation mask"
            mask_kw["relu_bits"] = xb
        if route != "F2_gemm_f32":            # (F(2x2,3x3) overwrites; the library refuses accumulate there)
            pre = torch.randn(1, h, w, cin, generator=g, device="cuda")
            acc = dg(out=pre.clone(), accumulate=True, **mask_kw)
            assert torch.equal(acc, pre + masked), "accumulate != pre + masked"
    for k, (mx, rms) in res.items():
        print(f"{RC.case_id(case):42s} {k:13s} max {mx:.2e}  rms {rms:.2e}  (tol {tol:.0e})")
        assert mx < tol, (RC.case_id(case), k, mx, tol)
    return res


def test_float64_reference_is_conv2d():
    """The reference itself: _conv64 == torch.nn.functional.conv2d in float64 on the CPU, forward and data-gradient."""
    g = torch.Generator().manual_seed(5)
    for h, w, cin, cout in ((7, 5, 64, 128), (9, 13, 32, 64)):
        x = torch.randn(1, h, w, cin, generator=g, dtype=torch.float64, requires_grad=True)
        wt = torch.randn(3, 3, cin, cout, generator=g, dtype=torch.float64)
        y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt.permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
        gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
        (y * gy).sum().backward()
        got = _conv64(x.detach().cuda(), wt.cuda()).cpu()
        assert (got - y.detach()).abs().max() < 1e-12 * y.abs().max()
        got = _conv64(gy.cuda(), wt.flip(0, 1).transpose(2, 3).cuda()).cpu()
        assert (got - x.grad).abs().max() < 1e-12 * x.grad.abs().max()


@pytest.mark.parametrize("case", RC.DEFAULT_CASES, ids=RC.case_id)
def test_route_matches_float64(case):
    check_case(case)


@pytest.mark.parametrize("group", sorted(RC.SWITCH_CASES))
def test_route_matches_float64_under_switches(group):
    env, cases = RC.SWITCH_CASES[group]
    out = subprocess.run([sys.executable, os.path.abspath(__file__), group], env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    done = json.loads(out.stdout.strip().splitlines()[-1])
    assert done == [RC.case_id(c) for c in cases]


if __name__ == "__main__":          # child of test_route_matches_float64_under_switches: one group under its switches
    group = sys.argv[1]
    ran = []
    for c in RC.SWITCH_CASES[group][1]:
        check_case(c)
        ran.append(RC.case_id(c))
    print(json.dumps(ran))
