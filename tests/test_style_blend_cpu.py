"""Style blending without a GPU: the --style_mix / --style_weights command line and its validation, the weights of a
StyleBlend, and the status codes of refused strotss_step_losses_blend_fwd_bwd calls (checked before anything launches)."""
import ctypes as C
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

EINVAL, EALIGN, ERANGE = -1, -2, -3
P = C.c_void_p(0x10000)          # "some buffer": non-null, never touched
WS = 1 << 30


def _args(*extra):
    import run_strotss as RS
    return RS.build_parser().parse_args(["c.jpg", "s.jpg", *extra])


def test_style_mix_flags_parse():
    a = _args("--style_mix", "a.jpg", "b.jpg", "--style_weights", "0.5", "0.3", "0.2")
    assert a.style_mix == ["a.jpg", "b.jpg"] and a.style_weights == [0.5, 0.3, 0.2]
    a = _args()
    assert a.style_mix is None and a.style_weights is None


def test_style_inputs_weights_and_zero_drop():
    import run_strotss as RS
    assert RS._style_inputs(_args()) == (["s.jpg"], [1.0])
    paths, w = RS._style_inputs(_args("--style_mix", "a.jpg"))                      # default: equal weights
    assert paths == ["s.jpg", "a.jpg"] and w == [0.5, 0.5]
    paths, w = RS._style_inputs(_args("--style_mix", "a.jpg", "b.jpg", "--style_weights", "3", "0", "1"))
    assert paths == ["s.jpg", "b.jpg"] and w == [0.75, 0.25]                        # zero weight: never loaded
    assert RS._style_inputs(_args("--style_mix", "a.jpg", "--style_weights", "1", "0")) == (["s.jpg"], [1.0])
    assert RS._style_inputs(_args("--style_mix", "a.jpg", "--style_weights", "0", "2")) == (["a.jpg"], [1.0])


@pytest.mark.parametrize("extra", [
    ("--style_mix", "a.jpg", "--style_weights", "1"),                               # count mismatch
    ("--style_mix", "a.jpg", "--style_weights", "1", "2", "3"),
    ("--style_weights", "1", "1"),
    ("--style_mix", "a.jpg", "--style_weights", "1", "-0.5"),                       # negative
    ("--style_mix", "a.jpg", "--style_weights", "0", "0"),                          # all zero
    ("--style_mix", "a.jpg", "--style_weights", "1", "nan"),                        # not finite
    ("--style_mix", "a.jpg", "b.jpg", "c.jpg", "d.jpg"),                            # more than STROTSS_MAX_STYLES
    ("--style_mix", "a.jpg", "--content_mask", "cm.jpg", "--style_mask", "sm.jpg"),  # blends with masks
    ("--style_mix", "a.jpg", "--strips"),                                           # blends with image strips
])
def test_style_inputs_refused(extra):
    import run_strotss as RS
    with pytest.raises(ValueError):
        RS._style_inputs(_args(*extra))


def test_style_blend_normalises_and_validates():
    from nn.engine import StyleBlend
    b = StyleBlend([None, None, None], [1.0, 2.0, 1.0])
    assert b.weights == [0.25, 0.5, 0.25]
    for targets, weights in (([None, None], [1.0]), ([None], [-1.0]), ([None, None], [0.0, 0.0]), ([None] * 5, [1.0] * 5)):
        with pytest.raises(ValueError):
            StyleBlend(targets, weights)


@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def _set(k=2, ns=1024, weight=1.0):
    from nn import _hip
    s = _hip.StyleSetT()
    s.n_styles = k
    for i in range(min(k, _hip.MAX_STYLES)):
        s.feats[i] = s.inv_norm[i] = s.panels[i] = s.mean[i] = s.cov[i] = P.value
        s.ns[i] = ns
        s.weight[i] = weight
    return s


def _call(lib, s, n=1024, d=2179, ld=2208, styles_ptr=True, gpred=P):
    f = C.c_float
    return lib.strotss_step_losses_blend_fwd_bwd(P, P, n, d, ld, C.byref(s) if styles_ptr else None, f(1), f(1), f(1), f(1),
                                                 gpred, P, P, P, P, P, WS, None)


def test_blend_entry_refuses_before_launching(lib):
    assert _call(lib, _set(), styles_ptr=False) == EINVAL                    # no style set
    assert _call(lib, _set(), gpred=None) == EINVAL                          # no gradient rows
    assert _call(lib, _set(k=0)) == ERANGE and _call(lib, _set(k=5)) == ERANGE
    s = _set(); s.feats[1] = None
    assert _call(lib, s) == EINVAL                                           # a style without rows
    assert _call(lib, _set(weight=-1.0)) == EINVAL
    assert _call(lib, _set(weight=float("nan"))) == EINVAL
    assert _call(lib, _set(weight=0.0)) == EINVAL                            # all weights zero
    assert _call(lib, _set(ns=0)) == EINVAL
    assert _call(lib, _set(ns=4096)) == ERANGE                               # more style rows than the tie lists hold
    assert _call(lib, _set(), ld=2180) == EALIGN                             # ld % 32 != 0
    assert _call(lib, _set(), ld=2176) == EINVAL                             # ld < d
    assert _call(lib, _set(), n=0) == EINVAL
    assert lib.strotss_step_losses_blend_workspace_bytes(C.byref(_set(k=5)), 1024, 2208) == 0
    assert lib.strotss_step_losses_blend_workspace_bytes(C.byref(_set(k=3)), 1024, 2208) > \
        lib.strotss_step_losses_blend_workspace_bytes(C.byref(_set(k=2)), 1024, 2208) > 0
    # one style: the single-style call's workspace
    one = _set(k=1, ns=1000)
    assert lib.strotss_step_losses_blend_workspace_bytes(C.byref(one), 1024, 2208) == \
        lib.strotss_step_losses_workspace_bytes(1000, 1024, 2208)


def test_blend_entry_refuses_without_the_x3_core(lib):
    """STROTSS_X3=0 switches the bf16x3 core off for the process (read once by the library): the blended call, like the
    single-style one, is then refused with STROTSS_EINVAL after every other check passed."""
    code = ("import sys; sys.path[:0] = [%r, %r]; import test_style_blend_cpu as T; from nn import _hip; "
            "lib = _hip.load_library(); print(T._call(lib, T._set()), T._call(lib, T._set(ns=4096)))"
            % (os.path.dirname(os.path.abspath(__file__)), PKG))
    env = dict(os.environ, STROTSS_X3="0")
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert out.returncode == 0, out.stderr
    assert out.stdout.split()[-2:] == [str(EINVAL), str(ERANGE)]
