"""CPU: the cases of tests/_route_cases.py still take the routes they are labelled with, so that the float64 parity of
tests/test_hip_conv_routes.py covers what it says it covers.  The policy is evaluated in child processes (the library
reads its switches once per process) that inherit this environment: run under a switch such as STROTSS_X3_MIN_TILES=0,
the default cases fail and are named."""
import json
import os
import subprocess
import sys

import _route_cases as RC

ROOT = RC.ROOT


def _misrouted(group=None):
    env = dict(os.environ)
    if group is not None:
        env.update(RC.SWITCH_CASES[group][0])
    sel = "RC.DEFAULT_CASES" if group is None else "RC.SWITCH_CASES[%r][1]" % group
    code = ("import json, sys; sys.path.insert(0, %r); import _route_cases as RC; print(json.dumps(RC.misrouted(%s)))"
            % (os.path.join(ROOT, "tests"), sel))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_default_cases_route_as_labelled():
    bad = _misrouted()
    assert not bad, "cases that no longer take their route (re-pick a shape): %s" % bad


def test_switch_cases_route_as_labelled():
    for group in RC.SWITCH_CASES:
        bad = _misrouted(group)
        assert not bad, "under %s: %s" % (RC.SWITCH_CASES[group][0], bad)


def test_every_route_appears_in_both_directions():
    cases = RC.DEFAULT_CASES + [c for _, cs in RC.SWITCH_CASES.values() for c in cs]
    assert all(c[0] in RC.ROUTES and c[1] in ("fwd", "dgrad") for c in cases)
    have = {(c[0], c[1]) for c in cases}
    want = {(r, d) for r in RC.ROUTES for d in ("fwd", "dgrad")}
    assert have == want, sorted(want - have)
    # the default policy alone reaches every route but the one-pass direct forward
    default = {(c[0], c[1]) for c in RC.DEFAULT_CASES}
    assert want - default == {("direct", "fwd")}
    assert len({RC.case_id(c) for c in cases}) == len(cases)


def test_cases_include_the_edges_kernels_get_wrong():
    cases = RC.DEFAULT_CASES + [c for _, cs in RC.SWITCH_CASES.values() for c in cs]
    for r in RC.ROUTES:          # a partial 4 x 4 tile at the bottom or right edge on every route
        assert any(c[0] == r and (c[2] % 4 or c[3] % 4) for c in cases), r

    def fused_items(h, w, cout):     # csrc/winograd_fused.hip: work items of 4 x 8 Winograd tiles x 32 channels
        return -(-(-(-h // 4)) // 4) * -(-(-(-w // 4)) // 8) * (cout // 32)
    n = [fused_items(h, w, co if d == "fwd" else ci) for r, d, h, w, ci, co in RC.DEFAULT_CASES if r == "F4_fused_f32"]
    assert any(k > 256 and k % 8 for k in n), n            # several items per workgroup, uneven per-XCD ranges


def test_cases_cover_every_layer_of_the_683x1024_scale():
    sys.path.insert(0, os.path.join(ROOT, "strotss-tensorflow_amd"))
    from nn import model as M
    h, w, layers = 683, 1024, set()
    for it in M.vgg_config("16"):
        if it == "pool":
            h, w = h // 2, w // 2
        elif it[1] != 3:
            layers.add((h, w, it[1], it[2]))
    for d in ("fwd", "dgrad"):
        assert layers <= {tuple(c[2:]) for c in RC.DEFAULT_CASES if c[1] == d}, d
