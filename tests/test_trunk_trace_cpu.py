"""CPU: the launches of VGGTrunk -- which wrapper of nn/_ops.py, in which order, with which buffers and flags -- are pinned to
tests/golden/trunk_trace.json for five image sizes, nine STROTSS_* switch settings and five calling modes (the generator,
tests/golden/make_trunk_trace.py, says how).  The trunk decides every layer's launches when it is built; forward() and
backward() only run that plan, so they may not ask the library anything: counted here as well.  One child process per switch
setting with all other STROTSS_* removed (the library reads its switches once per process), as tests/test_route_table.py."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_trunk_trace as T  # noqa: E402


@pytest.fixture(scope="module")
def run():
    """({setting: {cell: records}} regenerated, library calls of one forward + backward at 64 px), children side by side"""
    counter = T.start("", "T.library_calls()")
    return T.all_cells(), T.finish(counter)


@pytest.fixture(scope="module")
def traces(run):
    return run[0]


@pytest.fixture(scope="module")
def committed():
    with open(T.FIXTURE) as f:
        return json.load(f)


def test_launch_sequence_is_the_committed_one(traces, committed):
    assert sorted(traces) == sorted([""] + list(committed["sha256"])) == sorted(T.SETTINGS)
    assert sorted(traces[""]) == sorted(committed["default"])
    assert len(committed["default"]) == len(T.SIZES) * len(T.MODES) + len(T.EXTRA)
    for cell, idx in committed["default"].items():
        want, got = [committed["records"][i] for i in idx], traces[""][cell]
        for k, (a, b) in enumerate(zip(want, got)):
            assert a == b, "%s, record %d:\n  committed %s\n  now       %s" % (cell, k, a, b)
        assert len(want) == len(got), (cell, "committed %d records, now %d" % (len(want), len(got)), (want + got)[min(len(want), len(got))])
    for setting, cells in committed["sha256"].items():
        assert sorted(cells) == sorted(traces[setting]) and len(cells) == len(T.SIZES) * len(T.MODES)
        for cell, sha in cells.items():
            assert T.digest(traces[setting][cell]) == sha, (
                "%s, %s differs from the committed trace: `python tests/golden/make_trunk_trace.py %s %s` prints it in full, "
                "here and on the commit the fixture was made from" % (setting, cell, cell, setting))


def test_forward_and_backward_ask_the_library_nothing(run):
    assert run[1] == 0


def _count(records, name):
    return sum(r.startswith(name + "(") for r in records)


def test_fixture_is_not_vacuous(committed):
    """On the committed file alone: every switch moves the cell it is documented to matter for, every mode differs."""
    default = {cell: T.digest([committed["records"][i] for i in idx]) for cell, idx in committed["default"].items()}
    moved = {"STROTSS_WINOGRAD=0": "512x512", "STROTSS_WINOGRAD_TILE=2": "512x512", "STROTSS_RELU_BITS=0": "512x512",
             "STROTSS_PRESCATTER=0": "64x64", "STROTSS_POOL_IN_FINISH=0": "64x64", "STROTSS_CONV_VARIANT=1": "128x128",
             "STROTSS_DIRECT_MAX_TILES=0": "64x64", "STROTSS_PRESCATTER_MAX_PIXELS=1000000": "256x256"}
    assert sorted(moved) == sorted(committed["sha256"])
    for setting, size in moved.items():
        assert committed["sha256"][setting][size + " grad_all"] != default[size + " grad_all"], setting
    for size in ("64x64", "512x512"):
        by_mode = [default["%s %s" % (size, m)] for m in T.MODES]
        # (switching pre-scatter off on a live trunk gives the launches of a call without scatter_all; 512 px has none anyway)
        assert len(set(by_mode)) == (4 if size == "64x64" else 3), size
        assert default[size + " pre_off"] == default[size + " grad"]
    rec = {cell: [committed["records"][i] for i in idx] for cell, idx in committed["default"].items()}
    assert _count(rec["64x64 grad_all"], "maxpool2_fwd") == 0 and _count(rec["64x64 grad_all"], "conv3x3_dgrad_unpool") == 4
    assert _count(rec["64x64 halo"], "maxpool2_fwd") == 4 and _count(rec["64x64 halo"], "halo.refresh") == 25
    assert not any("relu_bits[" in r for r in rec["512x512 halo"]) and any("relu_bits[" in r for r in rec["512x512 grad_all"])
    assert _count(rec["vgg19 64x64 grad_all"], "conv3x3_relu_fwd") == 14 and _count(rec["taps2 64x64 grad_all"], "conv3x3_relu_fwd") == 5
    assert not any("dgrad" in r or "pool_codes" in r or "scatter" in r for r in rec["512x512 nograd"])


def test_switches_move_the_launches_as_documented(traces):
    t = traces
    for cell, records in t["STROTSS_RELU_BITS=0"].items():
        assert not any("relu_bits[" in r for r in records), cell
    off = t["STROTSS_POOL_IN_FINISH=0"]["64x64 grad_all"]
    assert _count(off, "maxpool2_fwd") == 4 and _count(off, "maxpool2_bwd") == 4 and _count(off, "conv3x3_dgrad_unpool") == 0
    for cell, records in t["STROTSS_WINOGRAD=0"].items():
        assert not any("winograd" in r for r in records), cell
    assert all("[4](36," not in r for records in t["STROTSS_WINOGRAD_TILE=2"].values() for r in records)
    assert any("[2](16," in r for r in t["STROTSS_WINOGRAD_TILE=2"]["512x512 grad_all"])
    assert all("scatter_all()" not in r for records in t["STROTSS_PRESCATTER=0"].values() for r in records)
    assert "scatter_all()" in t[""]["64x64 grad_all"] and "scatter_all()" in t[""]["128x128 grad_all"]
    assert "scatter_all()" not in t["STROTSS_CONV_VARIANT=1"]["128x128 grad_all"]       # a one-pass data-gradient cannot add
    assert "scatter_all()" in t["STROTSS_CONV_VARIANT=1"]["64x64 grad_all"]             # all split-K: it can
    big = t["STROTSS_PRESCATTER_MAX_PIXELS=1000000"]["256x256 grad_all"]                # pre-scatter with F(4x4) producers
    assert "scatter_all()" in big and "scatter_all()" not in t[""]["256x256 grad_all"]
    assert any(r.startswith("conv3x3_winograd_dgrad(") and "[4](36," in r and r.endswith("accumulate=True)") for r in big)
    odd = t["STROTSS_DIRECT_MAX_TILES=0"]["200x136 grad_all"]                            # both sides of the F(4x4) border
    assert any("[4](36," in r for r in odd) and any("[2](16," in r for r in odd) and not any(r.startswith("conv3x3_relu_fwd(") for r in odd)
    odd = t[""]["200x136 grad_all"]
    assert any("[4](36," in r for r in odd) and _count(odd, "conv3x3_relu_fwd") > 0 and not any("[2](16," in r for r in odd)
