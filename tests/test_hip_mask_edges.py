"""The mask kernels at their staging, chunk and grid-walk edges on the MI355X ("Mask kernel edges"):
strotss_refine_labels, strotss_kmeans_assign, strotss_kmeans_assign_prior, strotss_kmeans_update and strotss_label_warp at the
cases of tests/_mask_edge_cases.py, through that file's comparisons (tests/test_mask_edges_cpu.py shows that the cases reach
their edges and that each planted error fails the same comparisons).  The refinement and the update are called through the
library into sentinel-filled outputs and NaN-filled workspaces with spare room behind every buffer."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as KR  # noqa: E402
import _mask_edge_cases as M  # noqa: E402
import _track_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPARE = 64                                                            # elements behind every output
NAN_BITS = 0x7FC0BEEF                                                 # a quiet NaN that no kernel produces


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t.view(torch.int64) if t.dtype == torch.float64 else t


def _nan_bytes(nbytes):
    """a device buffer of nbytes + spare bytes, every 32-bit word the NaN above"""
    return torch.full(((nbytes + 4 * SPARE + 3) // 4,), NAN_BITS, dtype=torch.int32, device=DEV)


# ------------------------------------------------------------------ 1. refinement
def _refine_once(img, grid, k, radius, sigma_s, sigma_r):
    from nn import _hip
    lib = _hip.lib()
    (h, w), (gh, gw) = img.shape[:2], grid.shape
    nb = int(lib.strotss_refine_labels_workspace_bytes(h, w, gh, gw))
    assert nb >= gh * gw * 12
    label = torch.full((h * w + SPARE,), M.LABEL_SENTINEL, dtype=torch.int32, device=DEV)
    count = torch.full((k + SPARE,), M.COUNT_SENTINEL, dtype=torch.int32, device=DEV)
    best = torch.full((h * w + SPARE,), M.VOTE_SENTINEL, dtype=torch.float64, device=DEV)
    second = torch.full((h * w + SPARE,), M.VOTE_SENTINEL, dtype=torch.float64, device=DEV)
    ws = _nan_bytes(nb)
    _hip.check(lib.strotss_refine_labels(img.data_ptr(), h, w, grid.data_ptr(), gh, gw, k, radius, sigma_s, sigma_r,
                                         label.data_ptr(), best.data_ptr(), second.data_ptr(), count.data_ptr(), ws.data_ptr(), nb,
                                         _hip.stream_ptr()), "refine_labels")
    torch.cuda.synchronize()
    return label, count, best, second, ws


@pytest.mark.parametrize("name", M.REFINE_CASES)
def test_refine_at_its_staging_and_walk_edges(name):
    img, grid, ref, (k, radius, sigma_s, sigma_r) = M.refine_case(name)
    (h, w), (gh, gw) = img.shape[:2], grid.shape
    imgd, gridd = _dev(img), _dev(grid, torch.int32)
    first = _refine_once(imgd, gridd, k, radius, sigma_s, sigma_r)
    again = _refine_once(imgd, gridd, k, radius, sigma_s, sigma_r)
    for a, b in zip(first, again):                                    # the same bits, workspace and spare room included
        assert torch.equal(_bits(a), _bits(b))
    label, count, best, second, ws = (t.cpu().numpy() for t in first)
    got = dict(label=label[:h * w].reshape(h, w), best=best[:h * w].reshape(h, w), second=second[:h * w].reshape(h, w),
               count=count[:k], mean=ws[:gh * gw * 3].view(np.float32).reshape(gh, gw, 3),
               guards=dict(label=(label[h * w:] == M.LABEL_SENTINEL).all(), count=(count[k:] == M.COUNT_SENTINEL).all(),
                           best=(best[h * w:] == M.VOTE_SENTINEL).all(), second=(second[h * w:] == M.VOTE_SENTINEL).all(),
                           workspace=(ws[gh * gw * 3:] == np.int32(NAN_BITS)).all()))
    fig = M.refine_figures(got, ref, k, sigma_r)
    print(f"{name}: best {fig['best']:.3g} and second {fig['second']:.3g} of the bound, {int((got['label'] != ref['label']).sum())} "
          f"labels differ from the reference's, counts {got['count'].tolist()}")
    assert M.refine_failures(fig) == []
    assert not np.isnan(got["mean"]).any() and (got["best"] != M.VOTE_SENTINEL).all() and (got["second"] != M.VOTE_SENTINEL).all()


# ------------------------------------------------------------------ 2. assignment
@pytest.mark.parametrize("d", M.ASSIGN_D)
def test_assign_at_every_half_chunk_and_kp_edge(d):
    from nn import _ops
    worst = dict(best=0.0, second=0.0)
    for k in M.ASSIGN_K:
        x, inv, c32, prior = M.assign_data(d, k)
        xd, invd, cd = _dev(x), _dev(inv), _dev(c32)
        pd, nod = _dev(prior, torch.int32), _dev(np.full_like(prior, -1), torch.int32)
        for n in M.ASSIGN_N:
            plain = _ops.kmeans_assign(xd, invd, n, d, cd, k)
            zero = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, pd, 0.0)
            none = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, nod, M.ASSIGN_BETA)
            biased = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, pd, M.ASSIGN_BETA)
            for other in (zero, none):                                # no bias: the plain entry's bits
                assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(other, plain)), (k, n)
            for got, pr, beta in ((plain, None, 0.0), (biased, prior, M.ASSIGN_BETA)):
                fig = M.assign_figures(tuple(t.cpu().numpy() for t in got), M.assign_reference(x, inv, n, d, c32, pr, beta), d)
                assert M.assign_failures(fig) == [], (k, n, beta, fig)
                assert fig["within_E"] == 0                           # every margin is wide: the labels were compared exactly
                worst = {key: max(worst[key], fig[key]) for key in worst}
    print(f"assign d {d}: largest |best - ref| {worst['best']:.3f} and |second - ref| {worst['second']:.3f} of the tolerance "
          f"{KR.assign_bound(d) / 2 + M.U23:.2e}")


# ------------------------------------------------------------------ 3. update
@pytest.mark.parametrize("d", M.UPDATE_D)
def test_update_at_its_column_and_row_block_edges(d):
    from nn import _hip
    lib = _hip.lib()
    worst = 0.0
    for n in M.UPDATE_N:
        for k in M.UPDATE_K:
            x, inv, label, start, want, want_count = M.update_data(d, n, k)
            ld = x.shape[1]
            nb = int(lib.strotss_kmeans_update_workspace_bytes(n, ld, k))
            assert nb == M.row_blocks(n)[0] * k * ld * 8
            xd, invd, labd = _dev(x), _dev(inv), _dev(label, torch.int32)
            runs = []
            for _ in range(2):
                cd = torch.full((k * ld + SPARE,), 7.0, dtype=torch.float32, device=DEV)
                cd[:k * ld] = _dev(start).reshape(-1)
                count = torch.full((k + SPARE,), M.COUNT_SENTINEL, dtype=torch.int32, device=DEV)
                ws = _nan_bytes(nb)
                _hip.check(lib.strotss_kmeans_update(xd.data_ptr(), invd.data_ptr(), labd.data_ptr(), n, d, ld, k, cd.data_ptr(),
                                                     count.data_ptr(), ws.data_ptr(), nb, _hip.stream_ptr()), "kmeans_update")
                runs.append((cd, count, ws))
            torch.cuda.synchronize()
            assert torch.equal(_bits(runs[0][0]), _bits(runs[1][0])) and torch.equal(runs[0][1], runs[1][1])
            cd, count, ws = (t.cpu().numpy() for t in runs[0])
            assert (cd[k * ld:] == 7.0).all() and (count[k:] == M.COUNT_SENTINEL).all() and (ws[nb // 4:] == np.int32(NAN_BITS)).all()
            fig = M.update_figures(cd[:k * ld].reshape(k, ld), count[:k], want, want_count, start, d)
            assert M.update_failures(fig) == [], (n, k, fig)
            if k >= 2:
                assert want_count[k - 1] == 0
            worst = max(worst, fig["centres"])
    print(f"update d {d}: largest error {worst:.3f} of its bound")


# ------------------------------------------------------------------ 4. label warp
@pytest.mark.parametrize("shape", M.WARP_EDGE_SHAPES)
def test_label_warp_at_a_ragged_workgroup_and_on_the_borders(shape):
    from nn import _ops
    h, w, gh, gw = shape
    for name, grid, flow, cert in M.warp_edge_cases(h, w, gh, gw):
        want = TR.label_warp(grid, TR.WARP_K, flow, cert)
        g, f, c = _dev(grid, torch.int32), _dev(flow), None if cert is None else _dev(cert)
        got = _ops.label_warp(g, TR.WARP_K, f, c)
        again = _ops.label_warp(g, TR.WARP_K, f, c)
        assert got.dtype == torch.int32 and tuple(got.shape) == (gh, gw)
        assert np.array_equal(got.cpu().numpy(), want), name
        assert torch.equal(got, again), name
