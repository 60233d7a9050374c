"""GPU: every convolution route on data whose float64 result is the exact float32 answer (tests/_exact_cases.py), bit for
bit, and the bf16x3 core's m and l planes on wide operands under a bound that counts the output transform's roundings only.

Every case asserts its route, its exactness conditions (torch float64 on the device, none of the project's kernels) and its
non-triviality floors before it compares anything, and prints the figures it is judged by.  Integer family: forward
(activation, epilogue outputs requested at once, pooled copy, argmax codes by the header's definition, sign words),
data-gradient (plain, masked by activation, masked by sign words, accumulating onto an integer base, through the pool's
adjoint on the split-K route).  Wide family: the bf16x3 routes with f32 V and with panels.  The distance GEMM of the same
core with unit norms: C = 1 - x.y bit for bit.  The first layer with mean 0, std 1: (q - 0) * 1 and a 27-term integer sum,
exact (csrc/conv.hip), bit for bit.  The switch groups and the panel form run in a child process (switches are read once)."""
import json
import os
import subprocess
import sys

import pytest
import torch

import _exact_cases as E
import _route_cases as RC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ops():
    RC._model()
    from nn import _ops as ops
    return ops


def _assert_route(p):
    M = RC._model()
    now = M.conv_route(p.h, p.w, p.cin, p.cout, dgrad=p.direction == "dgrad")
    assert now == p.route, (p.id, "drifted to", now)
    tile = M.winograd_tile(p.h, p.w, p.cin, p.cout) if M.use_winograd(p.cin, p.cout) else 0
    assert tile == p.tile, (p.id, tile)


def _to_cuda(p):
    p.a = p.a.cuda()
    p.k_eff = p.k_eff.cuda()
    if p.bias is not None:
        p.bias = p.bias.cuda()
    return p


def _entry(p, ops):
    """The trunk's entry point and weight form for the problem (nn/model.py), and condition 1."""
    wt = p.wt
    if p.tile:
        g = wt.permute(3, 2, 0, 1) if p.direction == "fwd" else wt.flip(0, 1).permute(2, 3, 0, 1)
        u = ops.winograd_weights(g, p.tile)
        want = E.exact_u(p.k_eff, p.tile).reshape((p.tile + 2) ** 2, p.K, p.N).transpose(1, 2)
        assert torch.equal(u.double(), want), (p.id, "condition 1: U != (24 G) k (24 G)^T", int((u.double() != want).sum()))
        if p.direction == "fwd":
            return lambda **kw: ops.conv3x3_winograd_fwd(p.a, u, p.bias, **kw)
        return lambda **kw: ops.conv3x3_winograd_dgrad(p.a, u, p.cin, **kw)
    if p.direction == "fwd":
        w_tok = wt.permute(0, 1, 3, 2).reshape(9, p.cout, p.cin).contiguous()
        return lambda **kw: ops.conv3x3_relu_fwd(p.a, w_tok, p.bias, **kw)
    w_tik = wt.flip(0, 1).reshape(9, p.cin, p.cout).contiguous()
    p.w_tik = w_tik
    return lambda **kw: ops.conv3x3_dgrad(p.a, w_tik, p.cin, **kw)


def _nan(*shape):
    return torch.full(shape, float("nan"), device="cuda")          # an unwritten entry stays NaN and fails


def check_int_case(case):
    """One integer-family case, every form, bit for bit.  Returns the printed figures."""
    ops = _ops()
    p = _to_cuda(E.make_int_problem(case))
    _assert_route(p)
    extra = float(E.PRE_MAX) if p.direction == "dgrad" and p.route != "F2_gemm_f32" else 0.0
    if p.tile:
        fig, _, _ = E.winograd_conditions(p, extra=extra)
        E.assert_winograd_conditions(fig, p.id)
    else:
        fig = E.direct_conditions(p, extra=extra)
        assert fig["sum"] < 1.0, (p.id, "condition 6", fig)
    run = _entry(p, ops)
    conv = E.conv64(p.a, 576.0 * p.k_eff)
    h, w = p.h, p.w
    if p.direction == "fwd":
        pre = conv + p.bias.double()
        fig["pos"], fig["neg"] = E.assert_nontrivial(pre, p.id)
        ref = torch.relu(pre)
        got = run(out=_nan(1, h, w, p.cout))
        E.check_bitwise(got, ref, p.id + " fwd")
        extra_out = {}
        if p.route != "direct":                 # (the one-pass direct kernel has no pooling epilogue)
            extra_out["pool_out"] = _nan(1, h // 2, w // 2, p.cout)
            extra_out["pool_code"] = torch.full((1, h // 2, w // 2, p.cout), 9, dtype=torch.uint8, device="cuda")
        if p.route.startswith("F4"):
            extra_out["relu_bits_out"] = ops.relu_bits_buffer(h, w, p.cout, "cuda")
        if extra_out:                           # the trunk's call: everything the epilogue writes at once
            got2 = run(out=_nan(1, h, w, p.cout), **extra_out)
            E.check_bitwise(got2, ref, p.id + " fwd with every epilogue output")
        if "pool_out" in extra_out:
            pool, code = E.pool_reference(pre)
            fig["tied"] = E.tied_windows(pre)
            E.check_bitwise(extra_out["pool_out"], pool, p.id + " pool_out")
            E.check_codes(extra_out["pool_code"], code, p.id + " pool_code")
        if "relu_bits_out" in extra_out:
            E.check_sign_words(extra_out["relu_bits_out"], pre, p.id + " sign words")
            fig["zero_pre"] = float((pre == 0).double().mean())
    else:
        fig["pos"], fig["neg"] = E.assert_nontrivial(conv, p.id)
        x = p.mask_input().cuda()
        masked = conv * (x > 0)
        fig["masked_nonzero"] = float((masked != 0).double().mean())
        assert fig["masked_nonzero"] >= E.FLOOR, (p.id, "masked gradient", fig)
        E.check_bitwise(run(out=_nan(1, h, w, p.cin)), conv, p.id + " dgrad")
        E.check_bitwise(run(act_in=x, out=_nan(1, h, w, p.cin)), masked, p.id + " dgrad masked by act_in")
        mask_kw = {"act_in": x}
        if p.route.startswith("F4"):
            xb = E.sign_words(x)[0].int()
            E.check_bitwise(run(relu_bits=xb, out=_nan(1, h, w, p.cin)), masked, p.id + " dgrad masked by sign words")
            mask_kw["relu_bits"] = xb
        if p.route != "F2_gemm_f32":            # (F(2x2,3x3) overwrites; the library refuses accumulate there)
            base = p.base().cuda()
            E.check_bitwise(run(out=base.clone(), accumulate=True, **mask_kw), base.double() + masked, p.id + " dgrad accumulate")
        if p.route == "direct_splitk":          # through the pool's adjoint, from the codes
            code = torch.randint(0, 5, (1, h, w, p.cin), generator=E._gen(p.id + ":code"), dtype=torch.uint8).cuda()
            want = E.unpool_reference(conv, code)
            got = ops.conv3x3_dgrad_unpool(p.a, p.w_tik, p.cin, code, _nan(1, 2 * h, 2 * w, p.cin))
            E.check_bitwise(got, want, p.id + " dgrad_unpool")
            base2 = torch.randint(-E.PRE_MAX, E.PRE_MAX + 1, (1, 2 * h, 2 * w, p.cin), generator=E._gen(p.id + ":pre2")).float().cuda()
            got = ops.conv3x3_dgrad_unpool(p.a, p.w_tik, p.cin, code, base2.clone(), accumulate=True)
            E.check_bitwise(got, base2.double() + want, p.id + " dgrad_unpool accumulate")
    print(f"{p.id:44s} " + " ".join(f"{k} {v:.3g}" for k, v in fig.items()))
    return fig


def check_wide_case(shape, direction, kind):
    """One wide-family case: M exact, the plane shares above their floors, then every element within
    GAMMA9 (sum |A^T||M||A| + |bias|).  Returns (error / bound, m share, l share)."""
    ops = _ops()
    p = _to_cuda(E.make_wide_problem(shape, direction, kind))
    _assert_route(p)
    fig, Y, S = E.winograd_conditions(p)
    E.assert_winograd_conditions(fig, p.id, wide=True)
    sm, sl = E.plane_shares(p)
    fm, fl = E.WIDE_FLOORS[kind]
    assert sm >= fm and sl >= fl, (p.id, "plane shares", sm, sl, "floors", fm, fl)
    rows = list(range(-(-p.h // 4)))
    ref = E.untile(Y, p, rows)[:p.h][None]
    conv = E.conv64(p.a, 576.0 * p.k_eff)
    assert torch.equal(ref, conv), (p.id, "the float64 Winograd form is not the float64 convolution")
    bound = E.untile(S, p, rows)[:p.h][None]
    run = _entry(p, ops)
    if direction == "fwd":
        ref = ref + p.bias.double()
        E.assert_nontrivial(ref, p.id)
        bound = E.GAMMA9 * (bound + p.bias.double().abs())
        bits = ops.relu_bits_buffer(p.h, p.w, p.cout, "cuda")
        got = run(out=_nan(1, p.h, p.w, p.cout), relu_bits_out=bits)
        # max(., 0) is monotone and exact: the bound on the pre-activation holds for the activation
        worst = E.check_bound(got, torch.relu(ref), bound, p.id)
        sure = ref.abs() > bound                  # sign words where the sign is decided beyond the bound
        words, valid = E.sign_words(torch.where(sure, ref, torch.zeros_like(ref)))
        sure_w = E.sign_words(sure.double())[0]
        assert torch.equal(bits.long() & 0xFFFFFFFF & sure_w & valid, words), (p.id, "sign words")
    else:
        E.assert_nontrivial(ref, p.id)
        bound = E.GAMMA9 * bound
        worst = E.check_bound(run(out=_nan(1, p.h, p.w, p.cin)), ref, bound, p.id)
        x = p.mask_input().cuda()
        xb = E.sign_words(x)[0].int()
        worst = max(worst, E.check_bound(run(relu_bits=xb, out=_nan(1, p.h, p.w, p.cin)), ref * (x > 0), bound, p.id + " masked"))
    print(f"{p.id:52s} error/bound {worst:.3f}  m share {sm:.3f}  l share {sl:.3f}  sum|U||V| {fig['m']:.3f}  bits V {fig['bits_v']} U {fig['bits_u']}")
    return worst, sm, sl


@pytest.mark.parametrize("case", E.DEFAULT_CASES, ids=E.case_id)
def test_integer_case_is_bit_for_bit(case):
    check_int_case(case)


def _child(args, env):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, **env), capture_output=True,
                         text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("group", sorted(E.SWITCH_CASES))
def test_integer_cases_under_switches(group):
    env, cases = E.SWITCH_CASES[group]
    assert _child(["int", group], env) == [E.case_id(c) for c in cases]


def _wide_ids(group):
    return [E.wide_id(s, d, k) for s in E.WIDE_SHAPES if s[0] == group for d in ("fwd", "dgrad") for k in E.WIDE_KINDS]


@pytest.mark.parametrize("shape", [s for s in E.WIDE_SHAPES if s[0] is None], ids=lambda s: f"{s[1]}-{s[2]}x{s[3]}")
@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("kind", E.WIDE_KINDS)
def test_wide_case_within_the_output_transforms_roundings(shape, direction, kind):
    check_wide_case(shape, direction, kind)


def test_wide_cases_on_the_panel_form():
    """F4_x3_gemm_128 with V as x3 panels (STROTSS_X3_CONV_F32A=0) instead of f32 V split in registers."""
    assert _child(["wide", "panels"], {"STROTSS_X3_CONV_F32A": "0"}) == [
        E.wide_id(s, d, k) for s in E.WIDE_SHAPES if s[1] == "F4_x3_gemm_128" for d in ("fwd", "dgrad") for k in E.WIDE_KINDS]


def test_wide_cases_on_64_channels():
    env = E.SWITCH_CASES["x3_64_channels"][0]
    assert _child(["wide", "x3_64_channels"], env) == _wide_ids("x3_64_channels")


@pytest.mark.parametrize("shape", E.DIST_SHAPES, ids=lambda s: s[0])
@pytest.mark.parametrize("kind", E.DIST_KINDS)
def test_distance_gemm_is_bit_for_bit(shape, kind):
    """strotss_cosine_distance_x3 from strotss_row_inv_norm_x3's panels with rx = ry = 1: C = 1 - x y^T exactly; x == y gives
    an exactly symmetric matrix."""
    ops = _ops()
    label, n, ns = shape
    x, y = E.make_dist_rows(label, n, ns, kind)
    s, (sm, sl) = E.dist_conditions(x, y)
    z = E.dist_self_operand(x, y, kind)
    sxx = E.dist_conditions(z, z)[0]
    assert s < 1.0 and sxx < 1.0, (label, kind, "sum |x|_3 |y|_3 / 2^24", s, sxx)
    if kind != "dense":
        assert sm >= 0.5 and (sl >= 0.1 or kind == "both_mid"), (label, kind, "plane shares", sm, sl)
    ld = ops.pad32(E.DIST_D)

    def buf(v):
        b = torch.zeros(v.shape[0], ld, device="cuda")
        b[:, :E.DIST_D] = v.cuda()
        return b

    bx, by, bz = buf(x), buf(y), buf(z)
    nz = int(z.shape[0])
    px, py, pz = ops.row_inv_norm_x3(bx, n)[1], ops.row_inv_norm_x3(by, ns)[1], ops.row_inv_norm_x3(bz, nz)[1]
    one = torch.ones(ops.pad32(max(n, ns)), device="cuda")
    C = ops.cosine_distance_x3(px, one, n, py, one.clone(), ns, ld)[:, :ns]
    ref = 1.0 - bx.double() @ by.double().T
    assert float((ref != 1).double().mean()) > 0.5, (label, kind, "trivial products")
    E.check_bitwise(C.contiguous()[None], ref[None], f"distance {label} {kind}")
    D = ops.cosine_distance_x3(pz, one, nz, pz, one, nz, ld)[:, :nz]
    E.check_bitwise(D.contiguous()[None], (1.0 - bz.double() @ bz.double().T)[None], f"self distance {label} {kind}")
    assert torch.equal(D, D.T)
    print(f"distance {label:14s} {kind:9s} sum|x||y| {s:.3g} (self {sxx:.3g}) of 2^24  m share {sm:.3f}  l share {sl:.3f}")


@pytest.mark.parametrize("hw", [(683, 1024), (1024, 683), (1024, 1024), (42, 64), (61, 67), (5, 257)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_first_layer_is_bit_for_bit_on_integers(hw):
    """conv3x3_c3_fwd / conv3x3_c3_dgrad with mean 0 and std 1: the preprocess (q - 0) * (1 / 1) is exact, the sums hold
    27 (forward) and 9 * 64 (data-gradient) integer products below 2^24."""
    ops = _ops()
    h, w = hw
    tag = f"c3-{h}x{w}"
    img = torch.randint(0, 256, (1, h, w, 3), generator=E._gen(tag + ":img")).float().cuda()
    k = torch.randint(-9, 10, (3, 3, 3, 64), generator=E._gen(tag + ":k")).float().cuda()
    b = torch.randint(-99, 100, (64,), generator=E._gen(tag + ":b")).float().cuda()
    s = float(E.conv64(img, k.abs()).max()) + 99
    assert s < E.LIMIT
    pre = E.conv64(img, k) + b.double()
    pos, neg = E.assert_nontrivial(pre, tag)
    bits = ops.relu_bits_buffer(h, w, 64, "cuda")
    got = ops.conv3x3_c3_fwd(img, k.reshape(27, 64).contiguous(), b, out=_nan(1, h, w, 64), mean=(0.0, 0.0, 0.0), std=(1.0, 1.0, 1.0),
                             relu_bits_out=bits)
    E.check_bitwise(got, torch.relu(pre), tag + " fwd")
    E.check_sign_words(bits, pre, tag + " sign words")
    gy = E._relu_ints(E._gen(tag + ":gy"), (1, h, w, 64), 7, signed=True).cuda()
    ref = E.conv64(gy, k.flip(0, 1).transpose(2, 3))
    s2 = float(E.conv64(gy.abs(), k.flip(0, 1).transpose(2, 3).abs()).max()) + E.PRE_MAX
    assert s2 < E.LIMIT
    E.assert_nontrivial(ref, tag + " dgrad")
    w_bwd = k.flip(0, 1).reshape(9, 3, 64).contiguous()
    E.check_bitwise(ops.conv3x3_c3_dgrad(gy, w_bwd, _nan(1, h, w, 3), std=(1.0, 1.0, 1.0)), ref, tag + " dgrad")
    base = torch.randint(-E.PRE_MAX, E.PRE_MAX + 1, (1, h, w, 3), generator=E._gen(tag + ":pre")).float().cuda()
    E.check_bitwise(ops.conv3x3_c3_dgrad(gy, w_bwd, base.clone(), accumulate=True, std=(1.0, 1.0, 1.0)), base.double() + ref,
                    tag + " dgrad accumulate")
    print(f"{tag:14s} sum {s / E.LIMIT:.3g} / {s2 / E.LIMIT:.3g} of 2^24  pos {pos:.3f} neg {neg:.3f}")


if __name__ == "__main__":          # child process: one switch group's integer cases, or wide cases under this environment
    mode, group = sys.argv[1:3]
    ran = []
    if mode == "int":
        for c in E.SWITCH_CASES[group][1]:
            check_int_case(c)
            ran.append(E.case_id(c))
    else:
        shapes = [s for s in E.WIDE_SHAPES if (s[1] == "F4_x3_gemm_128" if group == "panels" else s[0] == group)]
        for s in shapes:
            for d in ("fwd", "dgrad"):
                for k in E.WIDE_KINDS:
                    check_wide_case(s, d, k)
                    ran.append(E.wide_id(s, d, k))
    print(json.dumps(ran))
