"""CPU checks of the hypercolumn test kit (no GPU): the reference of tests/_hypercol_ref.py against the oracle's sample_features
and its float64 autograd on every case of tests/_hypercol_cases.py (at a reduced channel count), the property every case was
built for, read off its tap table, and six planted errors in a float32 numpy stand-in for the kernels, each of which the
comparison functions of the GPU test (tests/_hypercol_ref.py: check_gather, check_adjoint, and 'no pixel without a tap
changes') must refuse."""
import numpy as np
import pytest
import torch

import _hypercol_cases as HC
import _hypercol_ref as R
from oracle import strotss_oracle as O

SMALL = (3, 2, 2, 2, 2, 2, 2, 2, 2, 2)             # channels of the oracle comparison: the taps do not depend on them
MID = (3, 8, 8, 8, 8, 8, 8, 8, 8, 8)


def test_the_cases_cover_what_the_kit_promises():
    sizes = {(c.h, c.w) for c in HC.CASES}
    assert sizes >= set(HC.ALL2) | set(HC.ODD)
    assert {(683, 911), (767, 1023), (341, 455), (100, 75), (75, 100), (97, 131)} <= {(c.h, c.w) for c in HC.CASES if c.kind == "draw"}
    assert {c.kind for c in HC.CASES} == {"draw", "edges", "float", "one_pixel", "two_pixels"}
    assert {c.n for c in HC.CASES} >= {1, 37, 1000, 1024}
    assert {(c.h, c.w) for c in HC.CASES if c.grad == "int"} >= {(683, 1024), (1024, 1024)}
    assert any(c.sample_range and c.window for c in HC.CASES) and any(c.sample_range and not c.window for c in HC.CASES)
    assert set(HC.DENSE_SWITCH) <= set(HC.LABELS) and len(HC.DENSE_SWITCH) >= 20
    assert R.D == 2179 and R.map_shapes(683, 1024)[-1] == (42, 64)


@pytest.mark.parametrize("hw", HC.ALL2 + HC.ODD, ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_divisor_chains(hw):
    shapes = R.map_shapes(*hw)
    chains = R.divisors(shapes)
    assert chains == O.map_divisors(shapes)
    flat = chains[-1]
    assert len(flat) == 4
    if hw in HC.ALL2:
        assert all(y == 2.0 for y in flat)
    else:
        assert any(y != 2.0 for y in flat)
    if hw in ((100, 75), (75, 100)):                 # the axis choice differs between the two
        assert R.divisors(R.map_shapes(100, 75))[-1] != [y for y in R.divisors(R.map_shapes(75, 100))[-1]]
    if hw == (97, 131):                              # non-2 divisors meet the dense blocks (maps of at most 64 pixels)
        assert shapes[-1] == (6, 8) and any(y != 2.0 for y in flat)


def _segments(ti, tw, sample_range=None):
    px, smp, w, seg = R.plan(ti, tw, sample_range)
    return len(px), (np.diff(seg).max() if len(seg) > 1 else 0)


@pytest.mark.parametrize("label", HC.LABELS)
def test_case_has_the_property_it_was_built_for(label):
    case = HC.BY_LABEL[label]
    shapes = R.map_shapes(case.h, case.w)
    idx = HC.indices(case)
    assert idx.dtype == np.float32 and idx.shape == (case.n, 2)
    assert idx[:, 0].min() >= 0 and idx[:, 0].max() <= case.h - 1 and idx[:, 1].min() >= 0 and idx[:, 1].max() <= case.w - 1
    table = R.taps(shapes, idx, True)
    for (ti, tw), (h, w) in zip(table, shapes):
        assert ti.min() >= 0 and ti.max() < h * w and tw.dtype == np.float32
    valid0, _ = _segments(*table[0])
    if case.kind in ("draw", "edges"):               # integer positions: one live tap per sample on the level-0 maps
        assert valid0 == case.n
    if case.kind == "edges":                         # a duplicated tap through the clip that still weighs something
        dup = [((ti[:, 0] == ti[:, 2]) & (tw[:, 2] != 0)).any() or ((ti[:, 0] == ti[:, 1]) & (tw[:, 1] != 0)).any() for ti, tw in table]
        assert any(dup)
        past = [(gx.max() > h - 1) or (gy.max() > w - 1) for (gx, gy), (h, w) in zip(R.coordinates(shapes, idx), shapes)]
        assert any(past) or (case.h, case.w) in ((85, 128), (42, 64))      # a coordinate past the last map row or column
    if case.kind == "float":                         # the plan runs full
        assert valid0 == 4 * case.n == R.PLAN_E
    if case.kind == "one_pixel":
        assert max(_segments(ti, tw)[1] for ti, tw in table) == R.PLAN_E
        assert _segments(*table[0]) == (case.n, case.n)
    if case.kind == "two_pixels":
        assert max(_segments(ti, tw)[1] for ti, tw in table) >= 512
        assert len(np.unique(table[0][0][table[0][1] != 0])) == 2
    if case.kind in ("one_pixel", "two_pixels") and shapes[-1][0] * shapes[-1][1] <= 64:
        live = (table[-1][1] != 0).any(1)            # every sample is listed by a dense block: the list at its capacity
        assert live.sum() == 1024
    if case.grad == "int":
        g = HC.gradient(case, R.D)
        assert np.array_equal(g, np.round(g)) and np.abs(g).max() <= 8 and np.array_equal(idx, np.floor(idx))
        assert all(y == 2.0 for y in R.divisors(shapes)[-1])
        for ti, tw in table:                         # weights are multiples of 1/256: every partial sum fits 24 bits
            assert np.array_equal(tw * 256, np.round(tw * 256))
    if case.sample_range:
        assert 0 < case.sample_range[0] < case.sample_range[1] < case.n
    if case.window:
        wins = HC.windows(case, shapes, R.LEVELS)
        assert all(0 <= r0 and rows > 0 and r0 + rows <= h for (r0, rows), (h, _) in zip(wins, shapes))
        full = R.taps(shapes, idx, True)
        for (ti, tw), (fi, fw), (r0, rows), (h, w) in zip(R.taps(shapes, idx, True, wins, False), full, wins, shapes):
            assert np.array_equal(tw, fw)            # clamped: nothing is dropped
            inside = (fi // w >= r0) & (fi // w < r0 + rows)
            assert np.array_equal(ti[inside], fi[inside] - r0 * w)
            assert np.array_equal(ti[~inside] // w, np.where(fi[~inside] // w < r0, 0, rows - 1)) and inside.any() and (~inside).any()
        for (ti, tw), (fi, fw) in zip(R.taps(shapes, idx, True, wins, True), R.rows_of_full_map(full, shapes, wins)):
            assert np.array_equal(tw, fw) and np.array_equal(ti[tw != 0], fi[fw != 0])


@pytest.mark.parametrize("label", HC.LABELS)
def test_reference_equals_the_oracle(label):
    """gather and adjoint of the reference against O.sample_features and its float64 autograd, to 1e-12: the float32 weights enter
    both as exact float64 values, so one differing tap index or weight bit would show at 1e-8 or more"""
    case = HC.BY_LABEL[label]
    shapes = R.map_shapes(case.h, case.w)
    idx = HC.indices(case)
    maps = [m.double() for m in HC.fill_maps(case, shapes, SMALL, "cpu")]
    fetch = lambda k, pix: maps[k].reshape(-1, SMALL[k])[torch.from_numpy(pix)].numpy()
    d = sum(SMALL)
    for bilinear in (True, False):
        ref, _ = R.gather(R.taps(shapes, idx, bilinear), SMALL, fetch, bilinear)
        want = O.sample_features(maps, idx, bilinear).numpy()
        assert np.abs(ref - want).max() <= (1e-12 if bilinear else 0.0)
    g = HC.gradient(case, d)
    if case.sample_range:
        g_used = np.zeros_like(g)
        g_used[case.sample_range[0]:case.sample_range[1]] = g[case.sample_range[0]:case.sample_range[1]]
    else:
        g_used = g
    leaves = [m.clone().requires_grad_(True) for m in maps]
    (O.sample_features(leaves, idx, True) * torch.from_numpy(g_used).double()).sum().backward()
    wins = HC.windows(case, shapes, R.LEVELS)
    if wins is None:
        table = R.taps(shapes, idx, True)
    else:                                            # dropped rows: the same rows of the whole maps' adjoint
        table = R.taps(shapes, idx, True, wins, True)
        fetch = lambda k, pix: maps[k][0, wins[k][0]:wins[k][0] + wins[k][1]].reshape(-1, SMALL[k])[torch.from_numpy(pix)].numpy()
    adjs = R.adjoint(table, SMALL, g, fetch, 1, case.sample_range)
    for k, (adj, leaf, m) in enumerate(zip(adjs, leaves, maps)):
        want = (leaf.grad * ((m > 0) if k >= 1 else 1.0))[0]
        if wins is not None:
            want = want[wins[k][0]:wins[k][0] + wins[k][1]]
        want = want.reshape(-1, SMALL[k]).numpy().copy()
        assert np.abs(adj.ref - want[adj.pix]).max() <= 1e-12 * max(1.0, np.abs(want).max()), k
        assert np.all((adj.m > 0) | (adj.ref == 0)) and np.all(adj.B >= np.abs(adj.ref) - 1e-12)
        want[adj.pix] = 0
        assert not want.any(), k                     # nothing lands outside the touched pixels


# ------------------------------------------------------------------ planted errors
def _value(k, pix, c, masked_from=1):
    v = np.sin(0.37 * pix[:, None] + 1.7 * np.arange(c)[None, :] + k).astype(np.float32)
    return np.maximum(v, 0) if k >= masked_from else v


def _base(k, pix, c):
    t = np.cos(0.11 * pix[:, None] + 0.7 * np.arange(c)[None, :] + k)
    return (np.sign(t) * (0.5 + 0.5 * np.abs(t)) * 2.0 ** -10).astype(np.float32)


def standin_taps(shapes, idx, bug=None):
    """the kernels' sample_tap in float32 numpy, written on its own, with a planted error"""
    f1 = np.float32(1)
    chains = O.map_divisors(shapes)
    out = []
    for (h, w), chain in zip(shapes, chains):
        gx, gy = idx[:, 0].astype(np.float32), idx[:, 1].astype(np.float32)
        if bug == "chain_applied_once":
            chain = chain[-1:]
        for y in chain:
            gx, gy = gx / np.float32(y), gy / np.float32(y)
        fx, fy = np.floor(gx), np.floor(gy)
        dx, dy = gx - fx, gy - fy
        wa, wb, wc, wd = (f1 - dx) * (f1 - dy), (f1 - dx) * dy, dx * (f1 - dy), dx * dy
        if bug == "wb_wc_swapped":
            wb, wc = wc, wb
        if bug == "clip_to_h":
            x0, y0 = np.clip(fx, 0, h).astype(np.int64) % h, np.clip(fy, 0, w).astype(np.int64) % w
        else:
            x0, y0 = np.clip(fx, 0, h - 1).astype(np.int64), np.clip(fy, 0, w - 1).astype(np.int64)
        x1, y1 = np.minimum(x0 + 1, h - 1), np.minimum(y0 + 1, w - 1)
        if bug == "duplicate_tap_dropped":
            wc, wd = np.where(x1 == x0, np.float32(0), wc), np.where(x1 == x0, np.float32(0), wd)
        out.append((np.stack([x0 * w + y0, x0 * w + y1, x1 * w + y0, x1 * w + y1], 1),
                    np.stack([wa, wb, wc, wd], 1).astype(np.float32)))
    return out


def standin_run(case, chans, bug=None, lost=None):
    """gather and atomic-style adjoint in float32 from the stand-in's taps, compared exactly as the GPU test compares the kernels.
    lost = (map, sample, tap, first channel): that contribution misses a 64-channel chunk."""
    shapes = R.map_shapes(case.h, case.w)
    idx, g = HC.indices(case), HC.gradient(case, sum(chans))
    off = R.offsets(chans)
    table = standin_taps(shapes, idx, bug)
    fetch = lambda k, pix: _value(k, pix, chans[k])
    ref_table = R.taps(shapes, idx, True)
    failures = []
    got = np.zeros((case.n, off[-1]), np.float32)
    for k, (ti, tw) in enumerate(table):
        v = [_value(k, ti[:, q], chans[k]) for q in range(4)]
        got[:, off[k]:off[k + 1]] = ((v[0] * tw[:, 0:1] + v[1] * tw[:, 1:2]) + v[2] * tw[:, 2:3]) + v[3] * tw[:, 3:4]
    ref, A = R.gather(ref_table, chans, fetch, True)
    try:
        R.check_gather(got, ref, A, True, "stand-in")
    except AssertionError as e:
        failures.append(("gather", str(e)))
    adjs = R.adjoint(ref_table, chans, g, fetch, 1)
    mask_from = 0 if bug == "mask_on_map_0" else 1
    for k, ((ti, tw), adj) in enumerate(zip(table, adjs)):
        c = chans[k]
        px, smp, w = R.entries(ti, tw)
        pix, inv = np.unique(px, return_inverse=True)
        buf = _base(k, pix, c)
        prod = w[:, None] * g[smp, off[k]:off[k] + c]
        if lost is not None and lost[0] == k:
            e = np.flatnonzero((smp == lost[1]) & (px == ti[lost[1], lost[2]]))[0]
            prod[e, lost[3]:lost[3] + 64] = 0
        if k >= mask_from:
            prod = prod * (_value(k, pix, c, mask_from)[inv] > 0)
        np.add.at(buf, inv, prod.astype(np.float32))
        try:
            extra = ~np.isin(pix, adj.pix)                           # 'pixels without a tap keep their bits'
            assert not (R.bits(buf[extra]) != R.bits(_base(k, pix[extra], c))).any(), f"map {k}: pixels without a tap changed"
            at = _base(k, adj.pix, c)
            pos = np.searchsorted(pix, adj.pix)
            found = (pos < len(pix)) & (pix[np.minimum(pos, len(pix) - 1)] == adj.pix) if len(pix) else np.zeros(len(adj.pix), bool)
            at[found] = buf[pos[found]]
            R.check_adjoint(at, _base(k, adj.pix, c), adj, f"stand-in map {k}")
        except AssertionError as e:
            failures.append((f"adjoint map {k}", str(e)))
    return failures


PLANTED = [("wb_wc_swapped", "100x75_float", ("gather", "adjoint")),
           ("chain_applied_once", "683x911_draw", ("gather", "adjoint")),
           ("clip_to_h", "683x1024_edges", ("gather", "adjoint")),
           ("duplicate_tap_dropped", "683x1024_edges", ("gather", "adjoint")),
           ("mask_on_map_0", "100x75_draw", ("adjoint",))]


@pytest.mark.parametrize("label", sorted({p[1] for p in PLANTED}))
def test_the_standin_without_an_error_passes(label):
    assert standin_run(HC.BY_LABEL[label], MID) == []


@pytest.mark.parametrize("bug,label,where", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_error_is_caught(bug, label, where):
    failures = standin_run(HC.BY_LABEL[label], MID, bug)
    for part in where:
        hit = [f for f in failures if f[0].startswith(part)]
        assert hit, f"planted error {bug} passed the {part} comparison"
        print(f"PLANTED {bug} caught by the {part} comparison: {hit[0][1][:160]}")
    if bug == "mask_on_map_0":
        assert [f[0] for f in failures] == ["adjoint map 0"]


def test_one_lost_sample_tap_contribution_on_the_2179_column_row_is_caught():
    """the shared-GPU failure of DESIGN.md section 6: one (sample, tap) contribution of one 64-channel chunk missing, at
    1024 x 1024 with the product's channels -- everything else exactly right"""
    case = HC.BY_LABEL["1024x1024_draw"]
    assert standin_run(case, R.CHANNELS) == []
    table = R.taps(R.map_shapes(case.h, case.w), HC.indices(case), True)
    s = 517
    tap = int(np.flatnonzero(table[9][1][s] != 0)[-1])
    failures = standin_run(case, R.CHANNELS, lost=(9, s, tap, 128))
    assert [f[0] for f in failures] == ["adjoint map 9"], failures
    print(f"PLANTED lost_sample_tap caught by the adjoint comparison: {failures[0][1][:160]}")
