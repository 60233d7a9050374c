"""Device side of tests/test_hip_pixel_path.py: runs the pixel-side kernels on a case of tests/_pixel_cases.py and compares EVERY
element with the float64 restatement of tests/_pixel_ref.py.  Each function returns the largest error / bound it met.

Run as a program (`python _pixel_worker.py h w`) it is the child process of the STROTSS_CONV_VARIANT=1 run: the switch is read
once per process, so the fallback first-layer kernels need a process of their own."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import _pixel_cases as PC
import _pixel_ref as R

DEV = "cuda"
NAN = float("nan")


def report(what, label, value):
    print(f"MEASURE pixel {what} {label} {value:.4f}", flush=True)


def dev(x):
    return torch.as_tensor(np.ascontiguousarray(x), device=DEV)


def host(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


def ops():
    from nn import _ops
    return _ops


# ------------------------------------------------------------------ resize and its adjoint
def resize_forward(x, oh, ow, what):
    """x (ih, iw, c) float32 on the host: plain, alpha = 1 with an addend, alpha = -1 with an addend"""
    ref, s = R.resize(x, oh, ow)
    add = PC.normal(ref.shape, "add", *ref.shape)
    xd, worst = dev(x)[None], 0.0
    for alpha, a in ((1.0, None), (1.0, add), (-1.0, add)):
        out = torch.full((1, oh, ow, x.shape[2]), NAN, device=DEV)
        ops().resize_bilinear(xd, oh, ow, alpha, None if a is None else dev(a)[None], out=out)
        want = alpha * ref + (0.0 if a is None else a.astype(np.float64))
        worst = max(worst, R.check(host(out)[0], want, R.resize_bound(s, a), f"resize {what} alpha={alpha} add={a is not None}"))
    return worst


def resize_adjoint(g, ih, iw, what):
    ref, b, m = R.adjoint(g, ih, iw)
    out = torch.full((1, ih, iw, g.shape[2]), NAN, device=DEV)
    ops().resize_bilinear_adjoint(dev(g)[None], ih, iw, out=out)
    got = host(out)[0]
    worst = R.check(got, ref, R.adjoint_bound(b, m), f"adjoint {what}")
    none = np.broadcast_to(m == 0, got.shape)
    assert R.plus_zero(got[none]), f"adjoint {what}: a pixel without a contributing output is not +0.0"
    return worst


def pyramid_forms(sizes, what, expect_fused=True):
    """fold and fold adjoint of one pyramid: the entry points' route, the fused forms bit for bit the level-by-level chain, and
    every stage of the chain against the float64 resize / adjoint of the GPU's own previous stage
    -> (worst resize ratio, worst adjoint ratio)"""
    o = ops()
    if expect_fused:
        assert R.fused_forms_fit(sizes), f"{what}: not launched, the CPU footprint check refuses it"
    pyr = PC.pyramid(sizes)
    pd = [dev(p)[None] for p in pyr]
    wf = wa = 0.0
    # the chain, stage by stage
    t = pd[-1]
    for k in range(len(sizes) - 2, -1, -1):
        h, w = sizes[k]
        nxt = torch.full((1, h, w, 3), NAN, device=DEV)
        o.resize_bilinear(t, h, w, 1.0, pd[k], out=nxt)
        ref, s = R.resize(host(t)[0], h, w)
        wf = max(wf, R.check(host(nxt)[0], ref + pyr[k].astype(np.float64), R.resize_bound(s, pyr[k]), f"fold {what} stage {k}"))
        t = nxt
    out = torch.full((1, *sizes[0], 3), NAN, device=DEV)
    got = o.fold_pyramid(pd, out)
    assert (got is not None) == R.host_admits_fold(sizes), f"{what}: the entry point's route differs from its documented rule"
    assert (got is not None) == expect_fused, f"{what}: fold_pyramid {'refused' if got is None else 'took'} the pyramid"
    if got is not None:
        assert same_bits(got, t), f"fold {what}: the one-launch fold differs from the chain"
    # the adjoint
    g0 = PC.normal((*sizes[0], 3), "g0", *sizes[0])
    chain = [dev(g0)[None]]
    for k in range(1, len(sizes)):
        h, w = sizes[k]
        nxt = torch.full((1, h, w, 3), NAN, device=DEV)
        o.resize_bilinear_adjoint(chain[-1], h, w, out=nxt)
        ref, b, m = R.adjoint(host(chain[-1])[0], h, w)
        wa = max(wa, R.check(host(nxt)[0], ref, R.adjoint_bound(b, m), f"fold adjoint {what} stage {k}"))
        chain.append(nxt)
    fused = [dev(g0)[None]] + [torch.full((1, h, w, 3), NAN, device=DEV) for h, w in sizes[1:]]
    assert o.fold_pyramid_adjoint(fused)
    for k, (a, b) in enumerate(zip(fused, chain)):
        assert same_bits(a, b), f"fold adjoint {what}: level {k} differs from the chain"
    return wf, wa


def laplacian_steps(h, w):
    """the two resizes of make_laplacian at one size: down (alpha = 1), and x - up(down) (alpha = -1, addend), and the
    adjoint of the down-resize -> (worst resize ratio, worst adjoint ratio)"""
    hd, wd = max(h // 2, 1), max(w // 2, 1)
    x = PC.image(h, w)
    o = ops()
    down = torch.full((1, hd, wd, 3), NAN, device=DEV)
    o.resize_bilinear(dev(x)[None], hd, wd, out=down)
    ref, s = R.resize(x, hd, wd)
    wf = R.check(host(down)[0], ref, R.resize_bound(s), f"down {h}x{w}")
    lap = torch.full((1, h, w, 3), NAN, device=DEV)
    o.resize_bilinear(down, h, w, -1.0, dev(x)[None], out=lap)
    ref, s = R.resize(host(down)[0], h, w)
    wf = max(wf, R.check(host(lap)[0], x.astype(np.float64) - ref, R.resize_bound(s, x), f"laplacian {h}x{w}"))
    wa = resize_adjoint(PC.normal((hd, wd, 3), "gd", h, w), h, w, f"of the down-resize {h}x{w}")
    return wf, wa


# ------------------------------------------------------------------ first layer
def first_layer_forward(h, w, law="uniform", cout=64, chunk=64):
    """-> (worst error / bound, fraction of sign bits left out of the float64 comparison)"""
    o = ops()
    img = PC.image(h, w, law)
    wt, b = R.first_layer_weights(cout)
    out = torch.full((1, h, w, cout), NAN, device=DEV)
    o.conv3x3_c3_fwd(dev(img)[None], dev(wt), dev(b), out=out)
    bits = torch.full((((h + 3) // 4) * ((w + 3) // 4), cout), -1, dtype=torch.int32, device=DEV)
    out_b = torch.full((1, h, w, cout), NAN, device=DEV)
    o.conv3x3_c3_fwd(dev(img)[None], dev(wt), dev(b), out=out_b, relu_bits_out=bits)
    assert same_bits(out, out_b), f"first layer {h}x{w}: the output changes with relu_bits_out"
    got = host(out)[0]
    signs = R.unpack_sign_words(host(bits), h, w)
    assert np.array_equal(signs, got > 0), f"first layer {h}x{w}: sign words differ from the kernel's own output"
    worst, left_out = 0.0, 0
    for r0 in range(0, h, chunk):
        r1 = min(h, r0 + chunk)
        pre, bound = R.first_layer(img, wt, b, rows=(r0, r1))
        worst = max(worst, R.check(got[r0:r1], np.maximum(pre, 0), bound, f"first layer {h}x{w} {law} cout={cout} rows {r0}.."))
        decided = np.abs(pre) > bound
        assert np.array_equal(signs[r0:r1][decided], (pre > 0)[decided]), f"first layer {h}x{w}: a decided sign bit is wrong"
        left_out += int((~decided).sum())
    frac = left_out / got.size
    assert frac <= 1e-3, f"first layer {h}x{w}: {frac} of the sign bits undecided"
    return worst, frac


def first_layer_dgrad(h, w, cout=64):
    o = ops()
    wt, _ = R.first_layer_weights(cout)
    g = PC.normal((h, w, cout), "dg", h, w)
    ref, bb = R.first_layer_dgrad(g, wt)
    w_tic = dev(R.flipped_weights(wt))
    out = torch.full((1, h, w, 3), NAN, device=DEV)
    o.conv3x3_c3_dgrad(dev(g)[None], w_tic, out)
    worst = R.check(host(out)[0], ref, R.DGRAD_K * R.U * bb, f"data-gradient {h}x{w} cout={cout}")
    base = PC.normal((h, w, 3), "dgbase", h, w) * np.float32(np.abs(ref).mean())        # the gradient's own size, never zero
    acc = dev(base)[None].clone()
    o.conv3x3_c3_dgrad(dev(g)[None], w_tic, acc, accumulate=True)
    want = base.astype(np.float64) + ref
    return max(worst, R.check(host(acc)[0], want, R.DGRAD_K * R.U * bb + R.U * np.abs(want), f"data-gradient {h}x{w} onto a base"))


# ------------------------------------------------------------------ max-pool
def maxpool(h, w, c):
    o = ops()
    x = PC.pool_input(h, w, c)
    mx, code = R.maxpool(x)
    ho, wo = h // 2, w // 2
    xd = dev(x)[None]
    out = torch.full((1, ho, wo, c), NAN, device=DEV)
    cd = torch.full((1, ho, wo, c), 255, dtype=torch.uint8, device=DEV)
    o.maxpool2_fwd(xd, out=out, code=cd)
    what = f"pool {h}x{w}x{c}"
    assert np.array_equal(host(out)[0].view(np.uint32), mx.view(np.uint32)), f"{what}: pooled values"
    assert np.array_equal(host(cd)[0], code), f"{what}: {int((host(cd)[0] != code).sum())} codes differ from their definition"
    plain = torch.full((1, ho, wo, c), NAN, device=DEV)
    o.maxpool2_fwd(xd, out=plain)
    assert same_bits(plain, out), f"{what}: values change with the code buffer"
    gout = PC.normal((ho, wo, c), "poolg", h, w, c)
    want = R.maxpool_bwd(code, gout, h, w)
    base = PC.pool_base(h, w, c)
    for name, kw in (("activation", {}), ("code", {"code": cd})):
        gin = torch.full((1, h, w, c), NAN, device=DEV)
        o.maxpool2_bwd(xd, dev(gout)[None], out=gin, **kw)
        assert np.array_equal(host(gin)[0].view(np.uint32), want.view(np.uint32)), f"{what}: backward by {name}"
        acc = dev(base)[None].clone()
        o.maxpool2_bwd(xd, dev(gout)[None], out=acc, accumulate=True, **kw)
        assert np.array_equal(host(acc)[0].view(np.uint32), (base + want).view(np.uint32)), f"{what}: accumulating backward by {name}"


# ------------------------------------------------------------------ rmsprop and the byte output
def rmsprop(name):
    o = ops()
    sizes = PC.RMSPROP_SETS[name]
    var = [dev(PC.normal((n,), "var", n, k)) for k, n in enumerate(sizes)]
    rms = [torch.zeros(n, device=DEV) for n in sizes]
    wr = wv = 0.0
    for step in range(PC.RMSPROP_STEPS):
        g = [PC.rmsprop_gradient(n, step, k) for k, n in enumerate(sizes)]
        before = [(host(v), host(r)) for v, r in zip(var, rms)]
        o.rmsprop_step(var, rms, [dev(x) for x in g], PC.LR, PC.RHO, PC.EPS)
        for k, (v0, r0) in enumerate(before):
            r, rb, v, vb = R.rmsprop(v0, r0, g[k], PC.LR, PC.RHO, PC.EPS)
            wr = max(wr, R.check(host(rms[k]), r, rb, f"rmsprop {name} step {step} tensor {k} rms"))
            wv = max(wv, R.check(host(var[k]), v, vb, f"rmsprop {name} step {step} tensor {k} var"))
    return wr, wv


def postprocess(n, law, plant):
    from oracle import strotss_oracle as O
    for q, x in enumerate(PC.postprocess_input(n, law, plant)):
        got = host(ops().postprocess(dev(x)[None]))[0]
        ref = O.postprocess(torch.from_numpy(x)[None])
        assert got.dtype == np.uint8 and np.array_equal(got, ref), f"byte output n={n} {law} {plant} {q}: {int((got != ref).sum())} bytes differ"


if __name__ == "__main__":
    h, w = int(sys.argv[1]), int(sys.argv[2])
    setting = os.environ.get("STROTSS_CONV_VARIANT", "default")
    report(f"first_layer_variant_{setting}", f"{h}x{w}", first_layer_forward(h, w)[0])
    report(f"dgrad_variant_{setting}", f"{h}x{w}", first_layer_dgrad(h, w))
    print("WORKER OK", flush=True)
