"""Device side of tests/test_hip_hypercol.py: builds a case of tests/_hypercol_cases.py on the GPU, calls the C ABI's gathers and
tap adjoints, and compares EVERY element with the reference of tests/_hypercol_ref.py -- the touched pixels on the host at the
derived bounds, all other elements on the device, bit for bit against what the buffer held before the call.

Run as a program (`python _hypercol_worker.py label,label,...`) it is the child process of the dense-block settings: the
atomic adjoint reads STROTSS_SCATTER_DENSE once per process, so each setting needs a process of its own."""
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import _hypercol_cases as HC
import _hypercol_ref as R

DEV = "cuda"
SENTINEL = 7.25
N_MAPS = len(R.CHANNELS)
PER_MAP = [(k, k + 1) for k in range(N_MAPS - 1, -1, -1)]          # the interleaved backward: one map per launch, deepest first
ALL_MAPS = [(0, N_MAPS)]                                           # the pre-scatter of the small scales: all ten in one launch
# strotss_hypercol_scatter_plan's layout per map, in 32-bit words (csrc/image.hip: PlanView)
PLAN_WORDS = 2 + (R.PLAN_E + 1) + 3 * R.PLAN_E + 1
PLAN_SEG, PLAN_PIX, PLAN_SMP, PLAN_W = 2, 2 + R.PLAN_E + 1, 2 + R.PLAN_E + 1 + R.PLAN_E, 2 + R.PLAN_E + 1 + 2 * R.PLAN_E


def report(what, label, value):
    print(f"MEASURE hypercol {what} {label} {value:.4f}", flush=True)


def pad32(v):
    return (v + 31) // 32 * 32


def same_bits(a, b):
    return bool(torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)))


class Problem:
    """one case on the device: maps, base, indices, gradients, descriptors and the reference's tap tables"""

    def __init__(self, case, chans=R.CHANNELS, levels=R.LEVELS):
        from nn import _hip, _ops
        self.hip, self.ops, self.case, self.chans = _hip, _ops, case, list(chans)
        self.full_shapes = R.map_shapes(case.h, case.w, levels)
        self.window = HC.windows(case, self.full_shapes, levels)
        self.shapes = self.full_shapes if self.window is None else [(rows, w) for (_, w), (_, rows) in
                                                                    zip(self.full_shapes, self.window)]
        self.maps = HC.fill_maps(case, self.full_shapes, chans, DEV)
        if self.window is not None:
            self.maps = [m[:, r0:r0 + rows].contiguous() for m, (r0, rows) in zip(self.maps, self.window)]
        self.base = HC.fill_base(case, self.shapes, chans, DEV)
        self.idx_host = HC.indices(case)
        self.n, self.d = case.n, sum(chans)
        self.ld, self.rows = pad32(self.d), pad32(case.n) + 32
        self.idx = torch.as_tensor(self.idx_host, device=DEV)
        self.g_host = HC.gradient(case, self.d)
        self.g = torch.zeros((self.rows, self.ld), dtype=torch.float32, device=DEV)
        self.g[:self.n, :self.d] = torch.as_tensor(self.g_host, device=DEV)
        self.divs = _ops.map_divisors(self.full_shapes)            # the product's own chain, against the reference's in the taps
        self.range_dev = None if case.sample_range is None else torch.tensor(case.sample_range, dtype=torch.int32, device=DEV)
        self._memo = {}

    def descriptor(self, maps, gmaps=None, drop=False, ranged=True):
        win = None if self.window is None else [(r0, fh) for (r0, _), (fh, _) in zip(self.window, self.full_shapes)]
        mt = self.hip.make_maps(maps, self.divs, gmaps, win, window_drop=drop)
        if ranged and self.range_dev is not None:
            mt.sample_range = self.range_dev.data_ptr()
        return mt

    def fetch(self, k, pix, maps=None):
        m = (maps or self.maps)[k]
        return m.view(-1, m.shape[-1])[torch.as_tensor(pix, device=DEV)].cpu().numpy()

    def taps(self, bilinear=True, drop=False):
        key = ("taps", bilinear, drop)
        if key not in self._memo:
            self._memo[key] = R.taps(self.full_shapes, self.idx_host, bilinear, self.window, drop)
        return self._memo[key]

    def adjoint_ref(self, drop=False):
        """drop: 'the same rows of the full-map adjoint', made from the whole maps' tap table"""
        key = ("adj", drop)
        if key not in self._memo:
            table = self.taps(True, False)
            if drop:
                table = R.rows_of_full_map(R.taps(self.full_shapes, self.idx_host, True), self.full_shapes, self.window)
            self._memo[key] = R.adjoint(table, self.chans, self.g_host, self.fetch, 1, self.case.sample_range)
        return self._memo[key]

    # ------------------------------------------------------------------ adjoints
    def base_for(self, form, drop=False):
        """the base a form adds onto: the case's, for the atomic form capped at B / m per element (tests/_hypercol_cases.py)"""
        if form != "atomic" or self.case.grad == "int":
            return self.base
        key = ("base_atomic", drop)
        if key not in self._memo:
            out = []
            for k, adj in enumerate(self.adjoint_ref(drop)):
                b = self.base[k].clone()
                if len(adj.pix):
                    pt = torch.as_tensor(adj.pix, device=DEV)
                    cur = b.view(-1, self.chans[k])[pt].cpu().numpy().astype(np.float64)
                    cap = np.where((adj.m >= 2) & (adj.B > 0), adj.B / np.maximum(adj.m, 1), np.inf)
                    new = np.sign(cur) * np.minimum(np.abs(cur), cap)
                    b.view(-1, self.chans[k])[pt] = torch.as_tensor(new.astype(np.float32), device=DEV)
                out.append(b)
            self._memo[key] = out
        return self._memo[key]

    def run_adjoint(self, form, ranges, drop=False):
        """-> (gradient maps after the launches onto the form's base, plan buffer or None)"""
        gm = [b.clone() for b in self.base_for(form, drop)]
        mt = self.descriptor(self.maps, gm, drop)
        plan = None
        if form == "sorted":
            nb = self.hip.lib().strotss_hypercol_scatter_plan_bytes(N_MAPS)
            assert nb == 4 * PLAN_WORDS * N_MAPS
            plan = torch.full((nb,), 255, dtype=torch.uint8, device=DEV)
            self.ops.hypercol_scatter_plan(mt, self.idx, plan)
        for b, e in ranges:
            if form == "sorted":
                self.ops.hypercol_scatter_sorted(mt, plan, self.n, self.g, relu_mask_from=1, map_begin=b, map_end=e)
            else:
                self.ops.hypercol_scatter(self.maps, None, self.idx, self.g, relu_mask_from=1, map_begin=b, map_end=e, maps_t=mt)
        torch.cuda.synchronize()
        return gm, plan

    def check_adjoint(self, gm, what, drop=False, form="sorted"):
        """every element of every gradient map; -> largest error / bound"""
        worst = 0.0
        base = self.base_for(form, drop)
        exact = self.case.grad == "int"
        for k, adj in enumerate(self.adjoint_ref(drop)):
            c = self.chans[k]
            got2, base2 = gm[k].view(-1, c), base[k].view(-1, c)
            pt = torch.as_tensor(adj.pix, device=DEV)
            changed = (got2.view(torch.int32) != base2.view(torch.int32)).any(1)
            changed[pt] = False
            assert not bool(changed.any()), f"{what} map {k}: {int(changed.sum())} pixels without a tap changed, first " \
                                            f"{int(changed.nonzero()[0])}"
            worst = max(worst, R.check_adjoint(got2[pt].cpu().numpy(), base2[pt].cpu().numpy(), adj, f"{what} map {k}", exact))
        return worst

    def check_plan(self, plan, drop=False):
        words = plan.view(torch.int32).cpu().numpy().reshape(N_MAPS, PLAN_WORDS)
        for k, (ti, tw) in enumerate(self.taps(True, drop)):
            px, smp, w, seg = R.plan(ti, tw, self.case.sample_range)
            wk, nseg, nvalid = words[k], len(seg) - 1, len(px)
            assert nseg == len(np.unique(px)), k
            assert wk[0] == nseg, (k, wk[0], nseg)                                   # one segment per touched pixel
            got_seg = wk[PLAN_SEG:PLAN_SEG + nseg + 1]
            assert np.all(np.diff(got_seg) > 0) and got_seg[-1] == nvalid, k          # monotone, ends at the valid count
            assert np.array_equal(got_seg, seg), k
            assert np.array_equal(wk[PLAN_PIX:PLAN_PIX + nvalid], px), k              # sorted by (pixel, sample, tap)
            assert np.array_equal(wk[PLAN_SMP:PLAN_SMP + nvalid], smp), k
            assert np.array_equal(wk[PLAN_W:PLAN_W + nvalid], R.bits(w)), k           # the table's weights, bit for bit

    # ------------------------------------------------------------------ gathers
    def _call_gather(self, mt, bilinear, ld=None, rows=None):
        out = torch.full((rows or self.rows, ld or self.ld), SENTINEL, dtype=torch.float32, device=DEV)
        self.hip.check(self.hip.lib().strotss_hypercol_gather(C.byref(mt), self.idx.data_ptr(), self.n, bilinear, out.data_ptr(),
                                                              out.shape[1], self.hip.stream_ptr()), "hypercol_gather")
        return out

    def check_gather_block(self, out, ref, A, bilinear, d, what, ranged):
        """rows of the sample range against the reference; every other row keeps the sentinel; the rows that were gathered have
        their padding columns cleared (the loss kernels read whole ld-wide rows and rely on it)"""
        s0, s1 = self.case.sample_range if (ranged and self.case.sample_range) else (0, self.n)
        s1 = min(s1, self.n)
        sent = torch.full_like(out, SENTINEL)
        assert same_bits(out[:s0], sent[:s0]) and same_bits(out[s1:], sent[s1:]), f"{what}: a row outside the samples changed"
        assert same_bits(out[s0:s1, d:], torch.zeros_like(out[s0:s1, d:])), f"{what}: padding columns of gathered rows not +0"
        return R.check_gather(out[s0:s1, :d].cpu().numpy(), ref[s0:s1], A[s0:s1], bilinear, what)

    def run_gathers(self):
        """the three gather entry points, bilinear and nearest; -> largest error / bound of the bilinear gathers"""
        lib, hip = self.hip.lib(), self.hip
        worst = 0.0
        tb, ta = self.descriptor(self.maps), self.descriptor(self.base, ranged=False)
        wmap = torch.randn((1, self.case.h, self.case.w, 1), device=DEV,
                           generator=torch.Generator(device=DEV).manual_seed(self.case.seed + 5))
        tw_ = hip.make_maps([wmap], [[]])
        for bilinear in (1, 0):
            table = self.taps(bool(bilinear))
            ref, A = R.gather(table, self.chans, self.fetch, bool(bilinear))
            one = self._call_gather(tb, bilinear)
            worst = max(worst, self.check_gather_block(one, ref, A, bilinear, self.d, f"gather bilinear={bilinear}", True))
            ref_a, A_a = R.gather(table, self.chans, lambda k, pix: self.fetch(k, pix, self.base), bool(bilinear))
            one_a = self._call_gather(ta, bilinear)
            worst = max(worst, self.check_gather_block(one_a, ref_a, A_a, bilinear, self.d, f"gather(a) bilinear={bilinear}", False))
            # the one-channel weight map: no divisors, no window
            wt = R.taps([(self.case.h, self.case.w)], self.idx_host, bool(bilinear))
            ref_w, A_w = R.gather(wt, [1], lambda k, pix: self.fetch(0, pix, [wmap]), bool(bilinear))
            one_w = self._call_gather(tw_, bilinear, ld=1)
            assert same_bits(one_w[self.n:], torch.full_like(one_w[self.n:], SENTINEL))
            worst = max(worst, R.check_gather(one_w[:self.n].cpu().numpy(), ref_w, A_w, bool(bilinear), "weight map"))
            for cw in (False, True):
                oa, ob = torch.full_like(one, SENTINEL), torch.full_like(one, SENTINEL)
                zero = torch.full_like(one, 3.0)
                if cw:
                    wout = torch.full((self.rows,), SENTINEL, dtype=torch.float32, device=DEV)
                    hip.check(lib.strotss_hypercol_gather2_cw(C.byref(ta), C.byref(tb), C.byref(tw_), self.idx.data_ptr(), self.n,
                                                              bilinear, oa.data_ptr(), ob.data_ptr(), self.ld, zero.data_ptr(),
                                                              self.rows, wout.data_ptr(), self.rows, hip.stream_ptr()), "gather2_cw")
                    assert same_bits(wout[:self.n], one_w[:self.n, 0]), "gather2_cw: weights differ from the single gather"
                    assert same_bits(wout[self.n:], torch.zeros_like(wout[self.n:])), "gather2_cw: weight rows >= n not +0"
                else:
                    hip.check(lib.strotss_hypercol_gather2(C.byref(ta), C.byref(tb), self.idx.data_ptr(), self.n, bilinear,
                                                           oa.data_ptr(), ob.data_ptr(), self.ld, zero.data_ptr(), self.rows,
                                                           hip.stream_ptr()), "gather2")
                torch.cuda.synchronize()
                name = "gather2_cw" if cw else "gather2"
                assert same_bits(oa, one_a) and same_bits(ob, one), f"{name} bilinear={bilinear}: differs from the single gather"
                assert same_bits(zero, torch.zeros_like(zero)), f"{name}: zero fill incomplete"
        return worst


def tap_table_by_value(case):
    """Gathers on ten one-channel maps whose value is the pixel's own linear index (exact in f32: at most 2^20 pixels): the
    nearest gather returns the tap index itself, bit for bit the reference table's; the bilinear one lies within 4u A of the
    table's weights times indices.  A wrong divisor chain or clip shows as (map, sample).  -> largest bilinear error / bound"""
    from nn import _hip, _ops
    shapes = R.map_shapes(case.h, case.w)
    idx_host = HC.indices(case)
    idx = torch.as_tensor(idx_host, device=DEV)
    maps = [torch.arange(h * w, dtype=torch.float32, device=DEV).view(1, h, w, 1) for h, w in shapes]
    mt = _hip.make_maps(maps, _ops.map_divisors(shapes))
    n, ld, worst = case.n, 32, 0.0
    for bilinear in (0, 1):
        out = torch.full((pad32(n) + 32, ld), SENTINEL, dtype=torch.float32, device=DEV)
        _hip.check(_hip.lib().strotss_hypercol_gather(C.byref(mt), idx.data_ptr(), n, bilinear, out.data_ptr(), ld,
                                                      _hip.stream_ptr()), "hypercol_gather")
        table = R.taps(shapes, idx_host, bool(bilinear))
        ref, A = R.gather(table, [1] * N_MAPS, lambda k, pix: pix.astype(np.float32)[:, None], bool(bilinear))
        if not bilinear:
            assert np.array_equal(ref, np.stack([ti[:, 0] for ti, _ in table], 1))
        worst = max(worst, R.check_gather(out[:n, :N_MAPS].cpu().numpy(), ref, A, bool(bilinear), f"index-coded bilinear={bilinear}"))
        assert same_bits(out[n:], torch.full_like(out[n:], SENTINEL))
        assert same_bits(out[:n, N_MAPS:], torch.zeros_like(out[:n, N_MAPS:]))
    return worst


def atomic_forms(label):
    """the atomic adjoint of one case through both of the engine's launch patterns; -> largest error / bound"""
    P = Problem(HC.BY_LABEL[label])
    worst = 0.0
    for name, ranges in (("per_map", PER_MAP), ("all_maps", ALL_MAPS)):
        gm, _ = P.run_adjoint("atomic", ranges)
        worst = max(worst, P.check_adjoint(gm, f"{label} atomic {name}", form="atomic"))
    return worst


if __name__ == "__main__":
    setting = os.environ.get("STROTSS_SCATTER_DENSE", "default")
    for label in sys.argv[1].split(","):
        report(f"atomic_dense_{setting}", label, atomic_forms(label))
    print("WORKER OK", flush=True)
