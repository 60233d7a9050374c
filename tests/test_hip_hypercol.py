"""Hypercolumn sampling at the shapes a step runs: strotss_hypercol_gather / _gather2 / _gather2_cw and the three tap adjoints
(_scatter with its dense blocks, _scatter_plan + _scatter_sorted) at every case of tests/_hypercol_cases.py -- the product's
ten maps (2179 columns) at every scale of the schedule, sizes whose divisor chains are not 2.0, clipped and duplicated taps,
float positions, collapsed index sets, small sample counts, sample ranges and row windows -- against the float64 restatement
of tests/_hypercol_ref.py.

Every element of every output is compared.  The only tolerances are the three derived ones of tests/_hypercol_ref.py: nearest
gathers and exact-sum cases bitwise, bilinear gathers within 4u A, adjoints within (m + 2)u B + u|base + ref|.  Outputs are
pre-filled (gather outputs with a sentinel, gradient maps with a seeded non-zero base, the plan with 0xFF bytes): pixels
without a tap, masked elements, rows >= n and rows outside a sample range keep their bits.  The padding columns (>= 2179) of a
row the gather WRITES are cleared by it -- the loss kernels read whole ld-wide rows -- so there the check is +0.0 bit for bit;
in every other row they keep the sentinel.  The atomic form alone adds onto a base capped at B / m where m >= 2, because its
intermediate sums round at the size of the base, which the bound does not count (tests/_hypercol_cases.py).  The measured worst error / bound per form is in DESIGN.md section 6."""
import os
import subprocess
import sys

import pytest
import torch

import _hypercol_cases as HC

pytestmark = pytest.mark.gpu

PLAIN = [l for l in HC.LABELS if l not in HC.WINDOWED]


@pytest.fixture(scope="module")
def W():
    import _hypercol_worker
    return _hypercol_worker


@pytest.fixture(scope="module", params=HC.LABELS, ids=[f"case_{l}" for l in HC.LABELS])
def P(request, W):
    p = W.Problem(HC.BY_LABEL[request.param])
    yield p
    del p
    torch.cuda.empty_cache()


@pytest.mark.parametrize("label", PLAIN)
def test_tap_table_by_value(W, label):
    W.report("tap_table_bilinear", label, W.tap_table_by_value(HC.BY_LABEL[label]))


def test_three_gather_entry_points(W, P):
    W.report("gather_bilinear", P.case.label, P.run_gathers())


def test_adjoint_forms_onto_a_base(W, P):
    """atomic (dense blocks at their default) and sorted adjoint, each one map per launch from the deepest down and all ten in
    one launch, onto the base; the sorted form's two runs have equal bits; the exact-sum cases equal the float64 result and
    each other bit for bit; a windowed case runs both with clamped rows and with dropped ones"""
    label = P.case.label
    for drop in ((False, True) if P.window is not None else (False,)):
        tag = f"{label} drop={int(drop)}" if P.window is not None else label
        runs = {}
        for form in ("atomic", "sorted"):
            for name, ranges in (("per_map", W.PER_MAP), ("all_maps", W.ALL_MAPS)):
                gm, plan = P.run_adjoint(form, ranges, drop)
                W.report(f"adjoint_{form}_{name}", tag.replace(" ", "_"), P.check_adjoint(gm, f"{tag} {form} {name}", drop, form))
                if plan is not None:
                    P.check_plan(plan, drop)
                runs[form, name] = gm
        for a, b in zip(runs["sorted", "per_map"], runs["sorted", "all_maps"]):
            assert W.same_bits(a, b), f"{tag}: two runs of the sorted adjoint differ"
        if label in HC.EXACT:
            for name in ("per_map", "all_maps"):
                for a, b in zip(runs["atomic", name], runs["sorted", name]):
                    assert W.same_bits(a, b), f"{tag}: atomic and sorted adjoint differ on exact sums"


@pytest.mark.parametrize("setting", ["0", "4096"])
def test_atomic_adjoint_with_the_dense_blocks_off_and_widened(setting):
    """STROTSS_SCATTER_DENSE=0 (atomics on every map) and =4096 (dense blocks up to the 64 x 64 map of the largest scale), each
    in a child process of its own (the switch is read once per process), through both launch patterns onto the base"""
    env = dict(os.environ, STROTSS_SCATTER_DENSE=setting)
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_hypercol_worker.py")
    out = subprocess.run([sys.executable, worker, ",".join(HC.DENSE_SWITCH)], env=env, capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0 and "WORKER OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]
    assert out.stdout.count("MEASURE") == len(HC.DENSE_SWITCH)
