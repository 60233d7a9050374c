"""Ownership of scratch memory on the GPU: a StepEngine and its trunk draw from the engine's own
nn._ops.Workspaces, so a live captured graph is indifferent to what the rest of the process asks of the module-level
instance or of another engine, the engine leaves the module-level instance alone, and its arena is released with it."""
import gc

import numpy as np
import pytest
import torch

import _transport_ref as TR
from _loss_harness import DEV
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

H = W = 64
N = 256


def _engine(P, **kw):
    from test_hip_transport import _engine as make          # the transport tests' engine on a step_problem
    return make(P, **kw)


def _indices(steps, seed):
    rng = np.random.default_rng(seed)
    idx = [[torch.from_numpy(O.make_indices(H, W, True, N, rng)).to(DEV)] for _ in range(steps)]
    assert all(int(i[0].shape[0]) == N for i in idx)            # every set has the captured count: each step below replays
    return idx


def _captured_run(P, transport, idx, between=lambda: None):
    """engine captured on idx[0], `between`, then one replay per index set -> variables, gradients, every step's scalars"""
    eng = _engine(P, transport=transport, deterministic=True)
    eng.capture_graph(idx[0])
    between()
    scalars = []
    for i in idx:
        eng.step(i)
        scalars.append(eng.scalars.clone())
    torch.cuda.synchronize()
    assert eng._graph is not None and eng.steps_done == len(idx)
    return [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + scalars


@pytest.mark.parametrize("transport", ["remd", "sinkhorn"])       # the grouped entry / the separate entries with the borrow
def test_a_live_graph_is_indifferent_to_larger_requests_elsewhere(transport):
    from nn import _ops
    P = TR.step_problem(H, W, N, 21)
    idx = _indices(3, 6)

    def between():
        big = TR.step_problem(2 * H, 2 * W, N, 22)
        other = _engine(big, transport=transport, deterministic=True)        # its trunk needs more scratch than A's
        other.step([torch.from_numpy(i).to(DEV) for i in big["idx"]])
        n, ld = 1024, other.ld                                               # more rows than any call of A's
        g = torch.Generator().manual_seed(3)
        x = torch.rand((n, ld), generator=g)
        x[:, other.d:] = 0
        x = x.to(DEV)
        _ops.selfsim_fwd_bwd(x, x.clone(), n, other.d, 1.0, torch.zeros_like(x), torch.zeros(4, device=DEV))
        _ops.moment_stats(x, n, other.d)
        torch.cuda.synchronize()

    disturbed = _captured_run(P, transport, idx, between)
    fresh = _captured_run(P, transport, idx)
    for a, b in zip(disturbed, fresh):
        assert torch.equal(a, b)


def test_the_engine_stays_out_of_the_module_level_instance():
    from nn import _ops
    P = TR.step_problem(H, W, N, 23)
    idx = _indices(2, 7)
    eng = _engine(P, transport="sinkhorn", deterministic=True)

    def module_state():
        return ({k: (b.data_ptr(), b.numel()) for k, b in _ops.workspaces.bufs.items()},
                {k: (b.data_ptr(), b.numel()) for k, b in _ops.workspaces.fixed.items()}, _ops.workspaces.selfsim_record)
    before = module_state()
    for i in idx:
        eng.step(i)
    eng.capture_graph(idx[0])
    for i in idx:
        eng.step(i)
    torch.cuda.synchronize()
    assert module_state() == before
    assert eng._ws.bufs and eng._ws.frozen and eng._ws.selfsim_record is not None
    assert eng.trunk.ws is eng._ws and eng._ws is not _ops.workspaces


@pytest.mark.parametrize("transport", ["remd", "sinkhorn"])
def test_an_eager_step_with_more_samples_than_the_captured_one_fits_the_frozen_arena(transport):
    P = TR.step_problem(H, W, N, 25)
    full = _indices(3, 9)
    idx = [[full[0][0][:200]], full[1], [full[2][0][:200]]]         # captured count, a larger one (eager), the captured one again
    finals = []
    for graph in (True, False):
        eng = _engine(P, transport=transport, deterministic=True)
        if graph:
            eng.capture_graph(idx[0])
            held = {k: (b.data_ptr(), b.numel()) for k, b in eng._ws.bufs.items()}
        for i in idx:
            eng.step(i)
        torch.cuda.synchronize()
        if graph:           # the warm-up sized the arena for sample_size samples: nothing grew, nothing moved
            assert eng._ws.frozen and {k: (b.data_ptr(), b.numel()) for k, b in eng._ws.bufs.items()} == held
        finals.append([v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()])
    for a, b in zip(*finals):
        assert torch.equal(a, b), "graph + eager vs eager"


def test_the_arena_is_released_with_its_engine():
    P = TR.step_problem(H, W, N, 24)
    idx = _indices(1, 8)[0]

    def cycle():
        """(bytes of the engine's arena, bytes allocated while it lives); the engine is garbage on return"""
        eng = _engine(P, deterministic=True)
        eng.step(idx)
        eng.capture_graph(idx)
        eng.step(idx)
        torch.cuda.synchronize()
        return sum(b.numel() for b in eng._ws.bufs.values()), torch.cuda.memory_allocated()

    def settled():
        gc.collect()
        torch.cuda.synchronize()
        return torch.cuda.memory_allocated()
    cycle()                     # the module-level instance (feature extraction, style statistics) takes its size once
    before = settled()
    arena, alive = cycle()
    after = settled()
    assert arena > 0 and alive >= before + arena
    assert after <= before      # nothing of the test's own was made in between: all of it is back
