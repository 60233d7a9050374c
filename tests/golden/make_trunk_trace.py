"""Writes tests/golden/trunk_trace.json: the sequence of library-wrapper calls, with every argument, that one
`VGGTrunk.forward` + `backward` makes -- per image size, STROTSS_* switch setting and calling mode.  No GPU: the trunk is built
on the CPU and the nine launch wrappers of `nn._ops` (plus `winograd_weights`) are replaced by recorders that launch nothing;
the construction-time questions to the library (`conv3x3_direct_splits`, `conv3x3_dgrad_accumulates`, the route query) are
host arithmetic and run for real.  tests/test_trunk_trace_cpu.py regenerates the file and compares, so a change to the trunk's
host side that is meant to leave its launches alone is held to exactly that.  Regenerate deliberately (from the commit whose
launch sequence is the yardstick) and say so in the commit:

    python tests/golden/make_trunk_trace.py              # writes the fixture
    python tests/golden/make_trunk_trace.py 64x64 grad_all STROTSS_WINOGRAD=0      # prints one cell in full

A record is `wrapper(arg=value, ...)` with every argument bound (`inspect.signature(...).bind(...).apply_defaults()`, so an
omitted `relu_bits` and `relu_bits=None` are one record; `ws=None`, the module-level workspaces that the trunk traced here
draws from, is left out, another instance would show) and each tensor replaced by the trunk buffer it is (`acts[3]`,
`grads[1]`, `gpools[0]`, `pool_codes[2]`, `relu_bits[4]`, `gimg`, `img`; a weight by kind, layer, tile and shape).
`halo.refresh(...)`, `scatter(li)` and `scatter_all()` are records of their own, in sequence, and so is the first time the trunk
takes a tile size out of a layer's `u_fwd` / `u_bwd` entry (`winograd_weights(u_fwd[5], tile_m=4)`: that is when the entry
transforms the weights; the replaced `_ops.winograd_weights` only hands out an empty tensor of the right shape).

Sizes: the square scales 64 .. 512 and 200 x 136, whose blocks hold 27200, 6800, 1700, 425 and 96 pixels: blocks 3 and 4 lie on
either side of the 1024-pixel border of F(4x4,3x3) (with STROTSS_DIRECT_MAX_TILES=0 the trunk runs F(4x4), F(2x2) and, on
block 1's 64 channels, the direct kernel side by side).  The file keeps the full records of the cells without switches (as
indices into one table of distinct records) and one SHA-256 of the records of every other cell."""
import hashlib, inspect, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "strotss-tensorflow_amd")]

WRAPPERS = ("conv3x3_winograd_fwd", "conv3x3_relu_fwd", "conv3x3_dgrad", "conv3x3_dgrad_unpool", "conv3x3_winograd_dgrad",
            "conv3x3_c3_fwd", "conv3x3_c3_dgrad", "maxpool2_fwd", "maxpool2_bwd")
SIZES = ((64, 64), (128, 128), (256, 256), (512, 512), (200, 136))
MODES = ("nograd", "grad_all", "grad", "pre_off", "halo")
#   nograd:   with_grad=False, forward only          grad_all: forward, backward(scatter, scatter_all)
#   grad:     forward, backward(scatter)             pre_off:  trunk.prescatter = False on the finished trunk, then as grad_all
#   halo:     a stub halo exchange, then as grad_all
SETTINGS = ("", "STROTSS_WINOGRAD=0", "STROTSS_WINOGRAD_TILE=2", "STROTSS_RELU_BITS=0", "STROTSS_PRESCATTER=0",
            "STROTSS_POOL_IN_FINISH=0", "STROTSS_CONV_VARIANT=1", "STROTSS_DIRECT_MAX_TILES=0",
            "STROTSS_PRESCATTER_MAX_PIXELS=1000000")
EXTRA = (("vgg19 64x64 grad_all", '19', None, (64, 64), "grad_all"),                 # only without switches
         ("taps2 64x64 grad_all", '16', ['block2_conv1', 'block3_conv2'], (64, 64), "grad_all"))
FIXTURE = os.path.join(ROOT, "tests", "golden", "trunk_trace.json")


class _NamedWeights:
    """stands in for a layer's `u_fwd` / `u_bwd` entry: names every tensor the trunk takes out of it and records the first
    time it asks for a tile size (that is when the weights are transformed)"""

    def __init__(self, inner, label, tracer):
        self.inner, self.label, self.tracer, self.seen = inner, label, tracer, set()

    def __getitem__(self, m):
        u = self.inner[m]
        if m not in self.seen:
            self.seen.add(m)
            self.tracer.records.append("winograd_weights(%s, tile_m=%d)" % (self.label, m))
        self.tracer.names[id(u)] = "%s[%d]%s" % (self.label, m, tuple(u.shape))
        return u


_params = {}        # (vgg_type, taps) -> (VGGParams, its own u_fwd / u_bwd entries): the weights are laid out once per process


class _Halo:
    def __init__(self, tracer):
        self.tracer = tracer

    def refresh(self, t, level):
        self.tracer.records.append("halo.refresh(%s, %r)" % (self.tracer.show(t), level))


class Tracer:
    """One trunk on the CPU with recorders for wrappers; `run()` fills `records`."""

    def __init__(self, size, mode, vgg_type='16', taps=None):
        import torch
        from nn import _ops, model as M
        self.torch, self.ops, self.records, self.names = torch, _ops, [], {}
        self.sigs = {n: inspect.signature(getattr(_ops, n)) for n in WRAPPERS}
        self.mode = mode
        h, w = size
        self.saved = {n: getattr(_ops, n) for n in WRAPPERS + ("winograd_weights",)}
        for n in WRAPPERS:
            setattr(_ops, n, self._recorder(n))
        _ops.winograd_weights = self._winograd_weights
        try:
            key = (vgg_type, tuple(taps or ()))
            if key not in _params:
                weights = [(torch.empty(3, 3, it[1], it[2]), torch.empty(it[2])) for it in M.vgg_config(vgg_type) if it != 'pool']
                p = M.VGGParams(weights, vgg_type, taps, device="cpu")
                _params[key] = (p, [{k: L[k] for k in ("u_fwd", "u_bwd") if k in L} for L in p.layers])
            self.params, lazies = _params[key]
            p = self.params
            for li, L in enumerate(p.layers):
                for k in ("w_fwd", "w_bwd", "bias"):
                    self.names[id(L[k])] = "%s[%d]%s" % (k, li, tuple(L[k].shape))
                for k, lazy in lazies[li].items():
                    L[k] = _NamedWeights(lazy, "%s[%d]" % (k, li), self)
            self.trunk = t = M.VGGTrunk(p, h, w, with_grad=mode != "nograd", halo=_Halo(self) if mode == "halo" else None)
        except BaseException:
            self.restore()
            raise
        self.img = torch.empty(1, h, w, 3)
        self.names[id(self.img)] = "img"
        for attr in ("acts", "pools", "grads", "gpools", "pool_codes", "relu_bits"):
            for i, b in enumerate(getattr(t, attr, [])):
                if b is not None:
                    self.names[id(b)] = "%s[%d]" % (attr, i)
        if mode != "nograd":
            self.names[id(t.gimg)] = "gimg"
        if mode == "pre_off":
            t.prescatter = False

    def restore(self):
        for n, f in self.saved.items():
            setattr(self.ops, n, f)

    def show(self, v):
        if isinstance(v, self.torch.Tensor):
            return self.names.get(id(v)) or "tensor%s:%s" % (tuple(v.shape), v.dtype)
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.show(x) for x in v) + ")"
        return repr(v)

    def _recorder(self, name):
        def rec(*a, **k):
            b = self.sigs[name].bind(*a, **k)
            b.apply_defaults()
            self.records.append("%s(%s)" % (name, ", ".join("%s=%s" % (n, self.show(v)) for n, v in b.arguments.items()
                                                             if not (n == "ws" and v is None))))
            return b.arguments.get("out", b.arguments.get("out_full", b.arguments.get("gimg")))
        return rec

    def _winograd_weights(self, g, tile_m=2, device=None):
        return self.torch.empty(((tile_m + 2) ** 2, int(g.shape[0]), int(g.shape[1])))

    def run(self):
        """forward (+ backward) on the finished trunk; -> records"""
        t = self.trunk
        try:
            t.forward(self.img)
            if self.mode != "nograd":
                scatter = lambda li: self.records.append("scatter(%d)" % li)
                scatter_all = lambda: self.records.append("scatter_all()")
                if self.mode == "grad":
                    t.backward(scatter)
                else:
                    t.backward(scatter, scatter_all)
        finally:
            self.restore()
        return self.records


def cells():
    """{cell name: records} of this process, under the STROTSS_* switches it was started with"""
    out = {}
    for size in SIZES:
        for mode in MODES:
            out["%dx%d %s" % (size[0], size[1], mode)] = Tracer(size, mode).run()
    if not [k for k in os.environ if k.startswith("STROTSS_")]:
        for name, vgg_type, taps, size, mode in EXTRA:
            out[name] = Tracer(size, mode, vgg_type, taps).run()
    return out


def library_calls(size=(64, 64), mode="grad_all"):
    """How many calls into the loaded library one forward + backward of a FINISHED trunk makes.  The recorders launch
    nothing, so every call counted is a question the trunk asks at step time."""
    from nn import _hip
    real, count = _hip.load_library(), [0]

    class Counting:
        def __getattr__(self, name):
            f = getattr(real, name)

            def call(*a):
                count[0] += 1
                return f(*a)
            return call
    tr = Tracer(size, mode)
    _hip._lib = Counting()
    try:
        tr.run()
    finally:
        _hip._lib = real
    return count[0]


def child_env(setting):
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    if setting:
        k, v = setting.split("=")
        env[k] = v
    return env


def start(setting, expr="T.cells()"):
    """a child process with only `setting` among the STROTSS_* variables (the library reads its switches once per process)
    that prints `expr` as JSON"""
    code = ("import json, sys; sys.path.insert(0, %r); import make_trunk_trace as T; print(json.dumps(%s))"
            % (os.path.dirname(os.path.abspath(__file__)), expr))
    return subprocess.Popen([sys.executable, "-c", code], env=child_env(setting), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                            text=True)


def finish(child):
    out, err = child.communicate(timeout=600)
    assert child.returncode == 0, err[-3000:]
    return json.loads(out.strip().splitlines()[-1])


def digest(records):
    return hashlib.sha256("\n".join(records).encode()).hexdigest()


def all_cells():
    """{setting: {cell: records}}, one child process per setting, side by side"""
    children = [(s, start(s)) for s in SETTINGS]
    return {s: finish(c) for s, c in children}


def fixture(traces):
    table, index = [], {}
    default = {}
    for cell, records in traces[""].items():
        for r in records:
            if r not in index:
                index[r] = len(table)
                table.append(r)
        default[cell] = [index[r] for r in records]
    return {"records": table, "default": default,
            "sha256": {s: {cell: digest(r) for cell, r in traces[s].items()} for s in SETTINGS if s}}


if __name__ == "__main__":
    if len(sys.argv) > 1:              # one cell in full: SIZE MODE [SWITCH=VALUE]
        setting = sys.argv[3] if len(sys.argv) > 3 else ""
        h, w = sys.argv[1].split("x")
        print("\n".join(finish(start(setting, "T.Tracer((%d, %d), %r).run()" % (int(h), int(w), sys.argv[2])))))
    else:
        with open(FIXTURE, "w") as f:
            json.dump(fixture(all_cells()), f, separators=(",", ":"))
            f.write("\n")
