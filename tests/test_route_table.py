"""CPU: the DEFAULT kernel routing of every generic VGG16 layer (forward and data-gradient) at the five BASELINE scales is
pinned to tests/golden/route_table.json.  The host policy is only nn/model.py's `use_winograd` / `winograd_tile` /
`direct_splitk`; behind it the library decides (csrc/winograd.hip `winograd43_route` is the statement, its launches dispatch
on it) and the host asks: `strotss_conv3x3_winograd_route`, `strotss_conv3x3_workspace_bytes`,
`strotss_step_losses_available`, `strotss_conv3x3_dgrad_can_accumulate`.  ~25 STROTSS_* switches and thresholds tuned by
A/B runs on single boxes move it: without this pin a policy regression would pass every parity test (all routes compute the
same convolution, model.py:44-55 of the reference).  Runs in child processes with the STROTSS_* variables removed (the
library reads them once per process)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _table(env_extra=None):
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    env.update(env_extra or {})
    code = ("import json, sys; sys.path.insert(0, %r); import make_route_table as T; print(json.dumps(T.table()))"
            % os.path.join(ROOT, "tests", "golden"))
    out = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_default_route_table_is_the_committed_one():
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "route_table.json")))
    got = _table()
    assert sorted(got) == sorted(want) == ["1024", "128", "256", "512", "64"]
    for scale in want:
        for w, g in zip(want[scale], got[scale]):
            assert w == g, (scale, w, g)
        assert len(want[scale]) == len(got[scale]) == 12
    # what DESIGN.md 4 says about the 1024-px scale: 8 launches of the fused kernel per step, block5 on 64 x 64 tiles
    fused = sum(r[5:].count("F4_fused_f32") for r in got["1024"])
    assert fused == 8 and all(r[5] == r[6] == "F4_x3_gemm_64" for r in got["1024"] if r[0].startswith("block5"))
    assert all(r[5] == r[6] == "direct_splitk" for r in got["64"])


def test_route_switches_move_the_table():
    """The pin is not vacuous: the documented switches change the routes."""
    off = _table({"STROTSS_X3": "0"})
    assert not any("x3" in r[5] or "x3" in r[6] for rows in off.values() for r in rows)
    nowino = _table({"STROTSS_WINOGRAD": "0"})
    assert all(r[5].startswith("direct") and r[6].startswith("direct") for rows in nowino.values() for r in rows)
    nofused = _table({"STROTSS_WINO_FUSED": "0"})
    assert not any("fused" in r[5] or "fused" in r[6] for rows in nofused.values() for r in rows)


LIBRARY_SWITCHES = ("STROTSS_X3", "STROTSS_X3_COST", "STROTSS_X3_MOMENT", "STROTSS_X3_CONV", "STROTSS_X3_MIN_TILES",
                    "STROTSS_X3_MIN_COUT", "STROTSS_WINO_FUSED", "STROTSS_WINO_FUSED_MAX_COUT")


def _start(expr, env_extra=None):
    """A child process with the STROTSS_* variables removed and `env_extra` set (the library reads a switch once per process)
    that imports the binding, `_ops` and `model` and prints `expr` as JSON."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    env.update(env_extra or {})
    code = ("import json, sys; sys.path.insert(0, %r); from nn import _hip, _ops, model; lib = _hip.load_library(); "
            "print(json.dumps(%s))" % (os.path.join(ROOT, "strotss-tensorflow_amd"), expr))
    return subprocess.Popen([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)


def _finish(child):
    out, err = child.communicate(timeout=300)
    assert child.returncode == 0, err[-2000:]
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.parametrize("value", ["", "0", "00", "1", " 1", "2", "false", "1x"])
def test_host_reads_the_library_switches_as_atoi_does(value, monkeypatch):
    """The switches the library reads with getenv + atoi / atol mean the same on the host: "", "00" and "false" are 0 on
    both sides (a host that took them for "on" would make the grouped loss call, which the library refuses with EINVAL).
    What a library switch DECIDES the host asks the library, so those answers are the library's own parse: one child
    process per (variable, value).  `env_int`, for the host-only switches, is held to atoi in this process."""
    import ctypes
    from nn import _ops
    libc = ctypes.CDLL(None)
    libc.atoi.argtypes, libc.atoi.restype = [ctypes.c_char_p], ctypes.c_int
    c = libc.atoi(value.encode())
    x3_conv = "_ops.winograd_x3_wanted(36, 512, 512, 64, 64)"                                  # block5 at 1024 px: bf16x3
    children = [(name, _start("_ops.step_losses_available()", {name: value}))
                for name in ("STROTSS_X3", "STROTSS_X3_COST", "STROTSS_X3_MOMENT")]
    children += [(name, _start(x3_conv, {name: value})) for name in ("STROTSS_X3", "STROTSS_X3_CONV")]
    for name in LIBRARY_SWITCHES + ("STROTSS_GROUPED_LOSSES",):
        monkeypatch.delenv(name, raising=False)
    assert _ops.step_losses_available() and _ops.winograd_x3_wanted(36, 512, 512, 64, 64)
    for name, child in children:
        assert _finish(child) == (c != 0), name
    for name in LIBRARY_SWITCHES:
        assert _ops.env_int(name, 7) == 7
        monkeypatch.setenv(name, value)
        assert _ops.env_int(name, 7) == c, name


def test_grouped_losses_switch_is_read_on_every_call(monkeypatch):
    """STROTSS_GROUPED_LOSSES is the host's own switch: tests flip it inside one process."""
    from nn import _ops
    monkeypatch.delenv("STROTSS_GROUPED_LOSSES", raising=False)
    assert _ops.step_losses_available()
    monkeypatch.setenv("STROTSS_GROUPED_LOSSES", "0")
    assert not _ops.step_losses_available()
    monkeypatch.setenv("STROTSS_GROUPED_LOSSES", "1")
    assert _ops.step_losses_available()


def test_host_and_library_cannot_disagree():
    """A switch the host never mirrored (the fused kernel then declines every layer): the host still makes the x3 panels
    exactly where the library runs the bf16x3 GEMMs.  (A host with a policy of its own said "the fused kernel takes it",
    made no panels, and the layer ended on F4_gemm_f32 against the library's own F4_x3_gemm_64.)"""
    ask = "[model.conv_route(170, 256, 128, 128), _ops.winograd_x3_wanted(36, 128, 128, 170, 256)]"
    switched, default = _start(ask, {"STROTSS_WINO_FUSED_MIN_ITEMS": "1000000"}), _start(ask)
    assert _finish(switched) == ["F4_x3_gemm_64", True]
    assert _finish(default) == ["F4_fused_f32", False]


def test_library_says_where_the_direct_data_gradient_accumulates():
    """strotss_conv3x3_dgrad(accumulate = 1): the one-pass kernel of STROTSS_CONV_VARIANT=1 refuses (launch_conv, EINVAL),
    the split-K form adds under every variant (its finish kernel does the adding, csrc/conv.hip conv_dispatch)."""
    import _route_cases as RC
    one_pass, splitk = ("direct", "dgrad", 21, 64, 512, 64), ("direct_splitk", "dgrad", 13, 17, 256, 256)
    assert one_pass in RC.DEFAULT_CASES and splitk in RC.DEFAULT_CASES
    # the data-gradient of cin -> cout is a convolution cout -> cin: the library's (h, w, cout, cin)
    ask = ("[lib.strotss_conv3x3_dgrad_can_accumulate(*a) for a in "
           "[(21, 64, 64, 512), (13, 17, 256, 256), (0, 64, 64, 512), (21, 64, 64, 96)]]")      # .., no map, cin % 64 != 0
    default, variant1 = _start(ask), _start(ask, {"STROTSS_CONV_VARIANT": "1"})
    assert _finish(default) == [1, 1, 0, 0]
    assert _finish(variant1) == [0, 1, 0, 0]
