"""The kernels at the pixel end of a step at the shapes a step has: bilinear resize and its adjoint, the one-launch fold and the
fold adjoint's pair launches, the first VGG layer and its data-gradient, the 2x2 max-pool and its backward, RMSprop and the byte
output, at every case of tests/_pixel_cases.py against the float64 restatements of tests/_pixel_ref.py.

Every element of every output is compared.  The only tolerances are the derived bounds of tests/_pixel_ref.py (resize
8u (S + |add|), adjoint (m + 4)u B, first layer 31u (sum |w p| + |b|), data-gradient 580u B, rmsprop 3u / 6u |delta| + u |var'|)
and bitwise equality (fused against level-by-level forms, max-pool values, codes and backward, sign words, byte output).  Outputs
are pre-filled with NaN (codes with 255, sign words with all ones): every element must be written.  The fused fold and adjoint
are launched only at pyramids whose footprints tests/_pixel_ref.py has shown to fit their LDS regions.  The measured worst
error / bound per kernel is in DESIGN.md section 6."""
import os
import subprocess
import sys

import pytest

import _pixel_cases as PC

pytestmark = pytest.mark.gpu


def _id(t):
    return "x".join(str(v) for v in t)


@pytest.fixture(scope="module")
def W():
    import _pixel_worker
    return _pixel_worker


@pytest.mark.parametrize("case", PC.RESIZE_RATIOS, ids=_id)
def test_resize_forward_ratios(W, case):
    ih, iw, oh, ow, c = case
    W.report("resize", _id(case), W.resize_forward(PC.image(ih, iw, c=c), oh, ow, _id(case)))


@pytest.mark.parametrize("case", PC.ADJOINT_RATIOS, ids=_id)
def test_resize_adjoint_ratios(W, case):
    ih, iw, oh, ow, c = case
    W.report("adjoint", _id(case), W.resize_adjoint(PC.normal((oh, ow, c), "adj", *case), ih, iw, _id(case)))


@pytest.mark.parametrize("hw", PC.IMAGE_SIZES + PC.SEGMENT_EDGES, ids=_id)
def test_pyramid_kernels_at_image_sizes(W, hw):
    """make_laplacian's two resizes, the fold and the fold adjoint (fused forms bit for bit the chain, every stage of the chain
    against float64) on the pyramid make_laplacian_pyramid builds from this size"""
    wf, wa = W.laplacian_steps(*hw)
    f, a = W.pyramid_forms(PC.chain(*hw), _id(hw))
    W.report("resize", _id(hw), max(wf, f))
    W.report("adjoint", _id(hw), max(wa, a))


@pytest.mark.parametrize("orientation", ["rows", "columns"])
def test_pyramid_kernels_at_every_length(W, orientation):
    """the axis sweep: every length 1 .. 2050 on one axis, 5 on the other"""
    rows = orientation == "rows"
    sizes = [(n, PC.SWEEP_OTHER) if rows else (PC.SWEEP_OTHER, n) for n in range(1, PC.SWEEP_MAX + 1)]
    assert set(sizes) <= set(PC.sweep_sizes())
    assert len(sizes) >= PC.SWEEP_MAX
    wf = wa = 0.0
    at_f = at_a = None
    for hw in sizes:
        f1, a1 = W.laplacian_steps(*hw)
        f2, a2 = W.pyramid_forms(PC.chain(*hw), _id(hw))
        if max(f1, f2) > wf:
            wf, at_f = max(f1, f2), hw
        if max(a1, a2) > wa:
            wa, at_a = max(a1, a2), hw
    W.report(f"resize_sweep_{orientation}", _id(at_f), wf)
    W.report(f"adjoint_sweep_{orientation}", _id(at_a), wa)


@pytest.mark.parametrize("k", range(len(PC.REFUSED_PYRAMIDS)))
def test_refused_pyramids_fall_back_and_stay_correct(W, k):
    """pyramids the one-launch fold refuses (asserted from the entry point's return value); the adjoint entry point walks them
    level by level inside: both still meet the float64 check and the chain bit for bit"""
    f, a = W.pyramid_forms(PC.REFUSED_PYRAMIDS[k], f"refused{k}", expect_fused=False)
    W.report("resize", f"refused{k}", f)
    W.report("adjoint", f"refused{k}", a)


@pytest.mark.parametrize("hw", PC.FIRST_LAYER_SIZES, ids=_id)
def test_first_layer_forward(W, hw):
    worst, frac = W.first_layer_forward(*hw)
    W.report("first_layer", _id(hw), worst)
    W.report("first_layer_undecided_signs", _id(hw), frac)


@pytest.mark.parametrize("hw", [(683, 1024), (170, 256), (17, 257), (100, 75)], ids=_id)
def test_first_layer_forward_exact_zero_and_one_blocks(W, hw):
    W.report("first_layer_blocks", _id(hw), W.first_layer_forward(*hw, law="blocks")[0])


@pytest.mark.parametrize("hw", PC.FIRST_LAYER_SIZES, ids=_id)
def test_first_layer_data_gradient(W, hw):
    W.report("dgrad", _id(hw), W.first_layer_dgrad(*hw))


def test_first_layer_fallback_kernels_32_channels(W):
    W.report("first_layer_cout32", "170x256", W.first_layer_forward(170, 256, cout=32)[0])
    W.report("dgrad_cout32", "170x256", W.first_layer_dgrad(170, 256, cout=32))


def test_first_layer_fallback_kernels_by_switch():
    """STROTSS_CONV_VARIANT=1 (read once per process): the plain kernels at 64 channels, in a child process"""
    env = dict(os.environ, STROTSS_CONV_VARIANT="1")
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_pixel_worker.py")
    out = subprocess.run([sys.executable, worker, "341", "512"], env=env, capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and "WORKER OK" in out.stdout, out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("hwc", PC.POOL_SHAPES, ids=_id)
def test_maxpool_values_codes_and_backward(W, hwc):
    W.maxpool(*hwc)


@pytest.mark.parametrize("name", list(PC.RMSPROP_SETS))
def test_rmsprop_three_steps(W, name):
    wr, wv = W.rmsprop(name)
    W.report("rmsprop_rms", name, wr)
    W.report("rmsprop_var", name, wv)


@pytest.mark.parametrize("plant", PC.POSTPROCESS_PLANTS)
@pytest.mark.parametrize("law", PC.POSTPROCESS_LAWS)
@pytest.mark.parametrize("n", PC.POSTPROCESS_LENGTHS)
def test_byte_output(W, n, law, plant):
    W.postprocess(n, law, plant)
