"""An independent restatement of hypercolumn sampling (csrc/image.hip: sample_tap, the three gathers, the three tap adjoints)
for tests/test_hip_hypercol.py and tests/test_hypercol_cases_cpu.py.  It never calls oracle.strotss_oracle.sample_features:
tests/test_hypercol_cases_cpu.py compares the two on every case.

The TAP TABLE is part of the specification, float32 operation by float32 operation: the sample coordinates are divided
cumulatively by the float32 divisor chain (one axis's ratio for both coordinates), then floor, clip and the four weight products,
all in float32.  IEEE division, subtraction and multiplication are correctly rounded on both sides, so the kernel's tap indices
and weights must equal the table's bit for bit.  What remains are sums, and the bounds below follow from their length alone
(u = 2^-24, the unit roundoff of float32):

  nearest gather     bitwise (a copy)
  bilinear gather    four products and three adds in some order, contracted or not:  |got - ref| <= 4u A,  A = sum |w||v|
  tap adjoint        m products added in some order, one more rounding where the dense blocks pre-add the coinciding taps of a
                     sample, and the add onto the base:  |got - (base + ref)| <= (m + 2)u B + u |base + ref|,  B = sum |w||g|
  exact sums         every product and partial sum representable: bitwise the float64 result

Only the pixels a tap touches are materialised: `fetch(k, pix)` returns the float32 rows of map k at the pixel ids `pix`."""
import numpy as np

U = 2.0 ** -24
CHANNELS = (3, 64, 64, 128, 128, 256, 256, 256, 512, 512)          # the step's ten maps: the image and nine trunk taps
LEVELS = (0, 0, 0, 1, 1, 2, 2, 2, 3, 4)                            # 2x2 VALID pools above each map (floor halving)
D = sum(CHANNELS)                                                  # 2179
PLAN_E = 4096                                                      # plan entries per map: 4 taps x <= 1024 samples


def map_shapes(h, w, levels=LEVELS):
    return [(h >> l, w >> l) for l in levels]


def offsets(chans):
    return np.concatenate([[0], np.cumsum(chans)]).astype(np.int64)


def divisors(shapes):
    """the divisor chain of every map: one more ratio whenever the height shrinks, taken on the axis that is fixed ONCE, at the
    first shrink: the height if the first shrunk height is a power of two, the width otherwise"""
    chains, cur, axis = [], [], None
    for i in range(len(shapes)):
        if i > 0 and shapes[i][0] < shapes[i - 1][0]:
            if axis is None:
                axis = 0 if shapes[i][0] & (shapes[i][0] - 1) == 0 else 1
            cur = cur + [shapes[i - 1][axis] / shapes[i][axis]]
        chains.append(list(cur))
    return chains


def coordinates(shapes, idx):
    """per map the float32 (row, col) coordinates after the cumulative float32 division"""
    idx = np.asarray(idx, np.float32)
    out = []
    for chain in divisors(shapes):
        gx, gy = idx[:, 0].copy(), idx[:, 1].copy()
        for y in chain:
            y32 = np.float32(y)
            gx = (gx / y32).astype(np.float32)
            gy = (gy / y32).astype(np.float32)
        out.append((gx, gy))
    return out


def taps(shapes, idx, bilinear, window=None, drop=False):
    """-> per map (int64 tap pixel ids (n, 4), float32 weights (n, 4)), taps in the order (x0,y0) (x0,y1) (x1,y0) (x1,y1).
    window[k] = (row0, rows): map k is held as its rows [row0, row0 + rows) only; the pixel ids then count inside the window,
    rows outside are clamped to its edge rows, or with `drop` keep their id but weigh nothing."""
    one = np.float32(1.0)
    out = []
    for k, ((h, w), (gx, gy)) in enumerate(zip(shapes, coordinates(shapes, idx))):
        n = len(gx)
        if bilinear:
            gxf, gyf = np.floor(gx), np.floor(gy)
            dx, dy = (gx - gxf).astype(np.float32), (gy - gyf).astype(np.float32)
            tw = np.stack([(one - dx) * (one - dy), (one - dx) * dy, dx * (one - dy), dx * dy], 1).astype(np.float32)
            x0 = np.clip(gxf, 0, h - 1).astype(np.int64)
            y0 = np.clip(gyf, 0, w - 1).astype(np.int64)
            x1, y1 = np.minimum(x0 + 1, h - 1), np.minimum(y0 + 1, w - 1)
        else:
            tw = np.zeros((n, 4), np.float32)
            tw[:, 0] = 1.0
            x0 = x1 = np.clip(gx, 0, h - 1).astype(np.int64)           # clip, then the truncating cast
            y0 = y1 = np.clip(gy, 0, w - 1).astype(np.int64)
        if window is not None and window[k] is not None:
            row0, rows = window[k]
            xa, xb = np.clip(x0 - row0, 0, rows - 1), np.clip(x1 - row0, 0, rows - 1)
            if drop and bilinear:
                tw[xa != x0 - row0, 0:2] = 0.0
                tw[xb != x1 - row0, 2:4] = 0.0
            x0, x1 = xa, xb
        out.append((np.stack([x0 * w + y0, x0 * w + y1, x1 * w + y0, x1 * w + y1], 1), tw))
    return out


def rows_of_full_map(tap_table, shapes, window):
    """the tap table of whole maps seen through a row window: ids renumbered inside the window, taps on other rows weigh nothing
    (the adjoint of these is 'the same rows of the full-map adjoint')"""
    out = []
    for (ti, tw), (h, w), (row0, rows) in zip(tap_table, shapes, window):
        r, c = ti // w, ti % w
        inside = (r >= row0) & (r < row0 + rows)
        out.append(((np.clip(r - row0, 0, rows - 1)) * w + c, np.where(inside, tw, np.float32(0.0)).astype(np.float32)))
    return out


def gather(tap_table, chans, fetch, bilinear):
    """-> float64 (n, D) reference and magnitude A = sum |w||v| (nearest: the value itself, A unused)"""
    n = tap_table[0][0].shape[0]
    off = offsets(chans)
    ref, A = np.zeros((n, off[-1])), np.zeros((n, off[-1]))
    for k, (ti, tw) in enumerate(tap_table):
        pix, inv = np.unique(ti, return_inverse=True)
        v = np.asarray(fetch(k, pix), np.float32).astype(np.float64)[inv.reshape(n, 4)]            # (n, 4, c)
        if bilinear:
            wv = tw.astype(np.float64)[:, :, None] * v
            ref[:, off[k]:off[k + 1]], A[:, off[k]:off[k + 1]] = wv.sum(1), np.abs(wv).sum(1)
        else:
            ref[:, off[k]:off[k + 1]] = v[:, 0]
    return ref, A


class Adjoint:
    """float64 adjoint of one map at its touched pixels: pix (p,) ascending pixel ids that receive an entry with a non-zero weight;
    ref, B (p, c) float64; m (p, c) entries per element (0 where the ReLU mask closes the element)"""

    def __init__(self, pix, ref, B, m):
        self.pix, self.ref, self.B, self.m = pix, ref, B, m


def entries(ti, tw, sample_range=None):
    """the (pixel, sample, tap weight) entries of a map that weigh something, in (sample, tap) order"""
    n = ti.shape[0]
    s0, s1 = (0, n) if sample_range is None else (max(0, sample_range[0]), min(n, sample_range[1]))
    keep = tw != 0
    keep[:s0] = False
    keep[s1:] = False
    smp = np.broadcast_to(np.arange(n)[:, None], (n, 4))
    return ti[keep], smp[keep], tw[keep]


def adjoint(tap_table, chans, g, fetch, relu_mask_from=1, sample_range=None):
    """g: (n, >= D) feature gradients (float32 values).  -> one Adjoint per map."""
    off = offsets(chans)
    g = np.asarray(g)
    out = []
    for k, (ti, tw) in enumerate(tap_table):
        c = chans[k]
        px, smp, w = entries(ti, tw, sample_range)
        pix, inv = np.unique(px, return_inverse=True)
        wg = w.astype(np.float64)[:, None] * g[smp, off[k]:off[k] + c].astype(np.float64)
        ref, B = np.zeros((len(pix), c)), np.zeros((len(pix), c))
        np.add.at(ref, inv, wg)
        np.add.at(B, inv, np.abs(wg))
        m = np.broadcast_to(np.bincount(inv, minlength=len(pix))[:, None], (len(pix), c)).copy()
        if k >= relu_mask_from and len(pix):
            live = np.asarray(fetch(k, pix), np.float32) > 0
            ref, B, m = ref * live, B * live, m * live
        out.append(Adjoint(pix, ref, B, m))
    return out


def plan(ti, tw, sample_range=None):
    """the sorted plan of one map: entries ordered by (pixel, sample, tap) -> pix, smp, w, seg_start (nseg + 1 values)"""
    n = ti.shape[0]
    px, smp, w = entries(ti, tw, sample_range)
    q = np.broadcast_to(np.arange(4)[None, :], (n, 4))
    s0, s1 = (0, n) if sample_range is None else (max(0, sample_range[0]), min(n, sample_range[1]))
    keep = tw != 0
    keep[:s0] = False
    keep[s1:] = False
    order = np.lexsort((q[keep], smp, px))
    px, smp, w = px[order], smp[order], w[order]
    heads = np.flatnonzero(np.concatenate([[True], px[1:] != px[:-1]])) if len(px) else np.zeros(0, np.int64)
    return px, smp, w, np.concatenate([heads, [len(px)]]).astype(np.int64)


# ------------------------------------------------------------------ the comparisons (the GPU test and the planted errors use these)
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def check_gather(got, ref, A, bilinear, what=""):
    """every element of the (n, D) block; -> largest error / bound"""
    got = np.asarray(got, np.float32)
    if not bilinear:
        bad = np.argwhere(bits(got) != bits(ref.astype(np.float32)))
        assert len(bad) == 0, f"{what}: nearest gather differs at {len(bad)} elements, first (sample, column) {bad[0]}"
        return 0.0
    err, bound = np.abs(got.astype(np.float64) - ref), 4 * U * A
    bad = np.argwhere(~(err <= bound))
    assert len(bad) == 0, (f"{what}: bilinear gather outside 4u A at {len(bad)} elements, first (sample, column) {bad[0]}: "
                           f"error {err[tuple(bad[0])]:.3e}, bound {bound[tuple(bad[0])]:.3e}")
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def check_adjoint(got, base, adj, what="", exact=False):
    """got, base: float32 (p, c) at adj.pix.  Elements without an entry keep the base's bits; the others lie within
    (m + 2)u B + u |base + ref| of base + ref, or equal it bit for bit with `exact`.  -> largest error / bound"""
    got, base = np.asarray(got, np.float32), np.asarray(base, np.float32)
    idle = adj.m == 0
    bad = np.argwhere(idle & (bits(got) != bits(base)))
    assert len(bad) == 0, f"{what}: {len(bad)} elements without an entry changed, first (touched pixel, channel) {bad[0]}"
    want = base.astype(np.float64) + adj.ref
    err = np.abs(got.astype(np.float64) - want)
    if exact:
        bad = np.argwhere(err != 0)
        assert len(bad) == 0, f"{what}: exact sums differ at {len(bad)} elements, first {bad[0]}: error {err[tuple(bad[0])]:.3e}"
        return 0.0
    bound = (adj.m + 2) * U * adj.B + U * np.abs(want)
    bad = np.argwhere(~(err <= bound))
    assert len(bad) == 0, (f"{what}: adjoint outside (m + 2)u B + u|base + ref| at {len(bad)} elements, first (touched pixel, "
                           f"channel) {bad[0]}: error {err[tuple(bad[0])]:.3e}, bound {bound[tuple(bad[0])]:.3e}, "
                           f"m {adj.m[tuple(bad[0])]}")
    live = ~idle
    return float((err[live] / bound[live]).max()) if live.any() else 0.0
