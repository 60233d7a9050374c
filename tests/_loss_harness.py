"""What every GPU test of a loss entry of the C ABI does around the call (tests/test_hip_loss_terms.py,
tests/test_hip_sinkhorn.py), as a plain module: padded device buffers, a first call on a zero buffer, then the cached
workspaces filled with NaN bytes (a read of workspace memory the call did not write shows), the gradient buffer holding a
seeded base (the entries ADD) with a sentinel in its padding rows and columns (left unchanged), and the two comparisons
against float64 (tests/_loss_ref.py), each printing a MEASURE line before it asserts."""
import numpy as np
import torch

import _loss_ref as LR

DEV = "cuda"
TOL_SCALAR, TOL_GRAD = LR.TOL_SCALAR, LR.TOL_GRAD
SENTINEL = 7.25


def report(what, case, value):
    print(f"MEASURE {what} {case} {value}")


def LC_pad(v):
    return (v + 31) // 32 * 32


def fbuf(x):
    n, d = x.shape
    b = torch.zeros((LC_pad(n), LC_pad(d)), dtype=torch.float32, device=DEV)
    b[:n, :d] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


def poison(ops):
    for b in ops.workspaces.bufs.values():
        b.fill_(255)


def gpred_base(n, d, scale, seed):
    g = torch.full((LC_pad(n), LC_pad(d)), SENTINEL, dtype=torch.float32)
    g[:n, :d] = torch.as_tensor(np.random.default_rng(seed).standard_normal((n, d)) * scale, dtype=torch.float32)
    return g.to(DEV)


def run_entry(ops, fn, n, d, scale, seed=0):
    """fn(gpred, loss4) once on a zero buffer (workspaces take their size; its gradient is returned for the duplicate-row
    check), then on NaN-filled workspaces into a seeded base with sentinel padding: (added gradient float64 [:n, :d],
    losses float64, gradient of the zero-buffer call)"""
    g0 = torch.zeros((LC_pad(n), LC_pad(d)), dtype=torch.float32, device=DEV)
    fn(g0, torch.zeros(4, 4, dtype=torch.float32, device=DEV))
    torch.cuda.synchronize()
    poison(ops)
    g = gpred_base(n, d, scale, seed)
    base = g.clone()
    loss = torch.zeros(4, 4, dtype=torch.float32, device=DEV)
    fn(g, loss)
    torch.cuda.synchronize()
    assert torch.equal(g[n:], base[n:]) and torch.equal(g[:, d:], base[:, d:]), "padding of gpred changed"
    got = (g.double() - base.double())[:n, :d].cpu().numpy()
    assert np.isfinite(got).all()
    return got, loss.double().cpu().numpy(), g0[:n, :d].cpu().numpy()


def check_scalar(what, label, got, ref):
    rel = abs(got - ref) / max(abs(ref), 1e-30)
    report(f"scalar:{what}", label, f"{rel:.3e}")
    assert abs(got - ref) <= TOL_SCALAR * abs(ref), (what, got, ref)


def check_gradient(what, label, got, ref, bound=None, tol=TOL_GRAD):
    ok, worst, rms = LR.check_grad(got, ref, bound, tol)
    report(f"grad:{what}", label, f"max {worst:.3e} rms {rms:.3e}")
    assert ok, (what, worst, rms)
