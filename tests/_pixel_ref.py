"""Float64 restatements of the kernels at the pixel end of a step, and the bounds their float32 results must meet, for
tests/test_hip_pixel_path.py and tests/test_pixel_cases_cpu.py: the bilinear resize and its adjoint (csrc/image.hip), the fused
fold and fold adjoint's footprints, the first VGG layer and its data-gradient, the 2x2 max-pool (csrc/conv.hip), RMSprop and the
byte output.  numpy on the CPU only.

u = 2^-24, the unit roundoff of float32.  Every bound is u times a count of roundings times the reference's own sum of absolute
terms; the counts are first-order (a sum of k roundings is charged k u, its u^2 terms are 1e-7 of that) and hold whether or not
the compiler contracts a multiply-add (contraction only removes roundings).

  resize        out = alpha * (top + (bot - top) ly) + add, top = tl + (tr - tl) lx, bot alike; alpha = +-1 is exact.
                The tap table (lo, hi, lerp) is float32 on both sides, bit for bit.  top: subtraction, product, sum = 3 roundings,
                each of a quantity of at most |tl| + |tr|; bot alike; the second lerp adds 3 more on at most the four values' sum
                S and carries the first two through with weight <= 1: <= 6u S.  The addend's sum is one more rounding at
                |out| <= S + |add|.   |got - ref| <= 7u (S + |add|) by this count; the suite uses the issue's 8u (S + |add|).
                S is the PLAIN sum of the four |tap values|: the weighted sum is not safe (with lerp near 1 the rounding of
                (tr - tl) is charged at |tl|, which the weight (1 - lerp) would hide).
  adjoint       gin[iy, ix] = sum_oy wy (sum_ox wx g).  A weight is 1 - lerp or lerp, or their float32 sum where both taps of
                an output fall on the same input pixel (the reference takes 1): one rounding per weight.  The row sum of mx
                products is charged mx + 1 (weight, products and adds), the column sum of my rows my + 1:
                (mx + my + 2)u B <= (m + 3)u B with m = mx my; the suite uses the issue's (m + 4)u B, B = sum |wy wx g|.
                Pixels without a contributing output have B = 0 and must be +0.0.
  first layer   p = (x - mean) * fl32(1 / std): two roundings of p; acc = bias, then 27 multiply-adds: bias is rounded 27 times,
                the first product 28 times (its own product and 27 sums): 30u (sum |w p| + |b|); the suite uses the issue's 31u.
                ReLU is 1-Lipschitz: the bound holds after it.
  data-gradient 576 products summed in some order, each term rounded at most 576 times, times fl32(1 / std): 577u B,
                B = fl32(1 / std) sum |w g|; the suite uses the issue's 580u B, plus u |base + ref| when it adds onto a base.
  max-pool      comparisons and copies: bitwise, the codes by their definition (first maximum in scan order, 4 if not positive)
  rmsprop       rms' = rho rms + (1 - rho) g g: 1 - rho is exact in float32 for rho in [0.5, 1]; g g, the product with 1 - rho
                and the sum round the second term three times, the first twice: 3u ref (all terms are non-negative).
                var' = var - lr g / (sqrt(rms') + eps): the reference takes the square root of ITS rms' (within 3u of the
                kernel's: 1.5u after the root), lr g, the root, the sum and the quotient round once each: 5.5u -> 6u |delta|,
                and the subtraction once: u |var'|.
  byte output   clip, subtract the minimum, IEEE divide, times 255, truncate: the same float32 operations in the oracle: bitwise"""
import functools

import numpy as np

from oracle import strotss_oracle as O

U = 2.0 ** -24
RESIZE_K, ADJOINT_K, FIRST_LAYER_K, DGRAD_K = 8, 4, 31, 580
FOLD_TILE, FOLD_REGION = 32, 24              # csrc/image.hip: the fold's image tile and the LDS region of the levels >= 1
ADJ2_T2, ADJ2_REGION = 8, 32                 # the adjoint pair's tile of the coarsest of its three levels, its LDS region


# ------------------------------------------------------------------ resize
def axis_table(in_size, out_size):
    """(lo, hi, lerp) of every output index: TF's float32 half-pixel table (the oracle's, which the kernel restates)"""
    return O._resize_axis_table(in_size, out_size)


def axis_weights(in_size, out_size):
    """(lo, hi, w_lo, w_hi) in float64; where both taps fall on one pixel the weight 1 goes to lo and 0 to hi"""
    lo, hi, l = axis_table(in_size, out_size)
    l = l.astype(np.float64)
    same = lo == hi
    return lo, hi, np.where(same, 1.0, 1.0 - l), np.where(same, 0.0, l)


def axis_matrix(in_size, out_size):
    """the dense (out, in) float64 matrix of one axis"""
    lo, hi, wl, wh = axis_weights(in_size, out_size)
    a = np.zeros((out_size, in_size))
    a[np.arange(out_size), lo] += wl
    a[np.arange(out_size), hi] += wh
    return a


def _apply(x, in_size, out_size, plain=False):
    """A x along axis 0 without storing A's zeros (two taps per row); plain: both weights 1 (the plain sum of |tap values|)"""
    lo, hi, wl, wh = axis_weights(in_size, out_size)
    shape = (-1,) + (1,) * (x.ndim - 1)
    if plain:
        return x[lo] + np.where(lo == hi, 0.0, 1.0).reshape(shape) * x[hi]
    return wl.reshape(shape) * x[lo] + wh.reshape(shape) * x[hi]


def resize(x, oh, ow):
    """x (ih, iw, c) float32 -> (A_y X A_x^T in float64, S = the plain sum of the four |tap values|); where two taps coincide
    the value is counted once"""
    x = np.asarray(x, np.float64)
    ih, iw = x.shape[:2]
    ref = _apply(_apply(x, ih, oh).swapaxes(0, 1), iw, ow).swapaxes(0, 1)
    s = _apply(_apply(np.abs(x), ih, oh, True).swapaxes(0, 1), iw, ow, True).swapaxes(0, 1)
    return ref, s


def resize_bound(s, add=None):
    return RESIZE_K * U * (s + (0.0 if add is None else np.abs(np.asarray(add, np.float64))))


def _apply_t(g, in_size, out_size, mode="w"):
    """A^T g along axis 0; mode "w": the weights, "count": 1 per contributing output"""
    lo, hi, wl, wh = axis_weights(in_size, out_size)
    if mode == "count":
        wl, wh = (wl != 0).astype(np.float64), (wh != 0).astype(np.float64)
    shape = (-1,) + (1,) * (g.ndim - 1)
    out = np.zeros((in_size,) + g.shape[1:])
    np.add.at(out, lo, wl.reshape(shape) * g)
    np.add.at(out, hi, wh.reshape(shape) * g)
    return out


def adjoint(g, ih, iw):
    """g (oh, ow, c) float32 -> (A_y^T G A_x in float64, B = sum |wy wx g|, m = the number of contributing outputs (ih, iw, 1))"""
    g = np.asarray(g, np.float64)
    oh, ow = g.shape[:2]
    ref = _apply_t(_apply_t(g, ih, oh).swapaxes(0, 1), iw, ow).swapaxes(0, 1)
    b = _apply_t(_apply_t(np.abs(g), ih, oh).swapaxes(0, 1), iw, ow).swapaxes(0, 1)
    my = _apply_t(np.ones((oh, 1)), ih, oh, "count")[:, 0]
    mx = _apply_t(np.ones((ow, 1)), iw, ow, "count")[:, 0]
    return ref, b, (my[:, None] * mx[None, :])[:, :, None]


def adjoint_bound(b, m):
    return (m + ADJOINT_K) * U * b


def check(got, ref, bound, what):
    """every element within its bound (an element whose bound is 0 must equal the reference, which is then 0);
    -> the largest error / bound"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{what}: {int((~np.isfinite(got)).sum())} elements are not finite"
    err = np.abs(got - ref)
    bound = np.broadcast_to(bound, err.shape)
    bad = err > bound
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0))),
                             err.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements over their bound, worst at {i}: got {got[i]!r} "
                             f"ref {ref[i]!r} error {err[i]:.3e} bound {bound[i]:.3e}")
    pos = bound > 0
    return float((err[pos] / bound[pos]).max()) if pos.any() else 0.0


def plus_zero(x):
    """whether every element is +0.0 bit for bit"""
    return bool((np.ascontiguousarray(x, np.float32).view(np.uint32) == 0).all())


# ------------------------------------------------------------------ footprints of the fused forms (one axis: the axes are independent)
def host_admits_fold(sizes):
    """the entry point's documented rule (include/strotss_hip.h: shrinking, halving or faster from level 1 on), as its worst case
    over tile positions: side' = min(n', floor(side n' / n) + 3) <= 24 from a 32-pixel tile on, per axis.  tests/
    test_hip_pixel_path.py holds this restatement to the entry point's own answer at every size it runs."""
    for axis in (0, 1):
        side = FOLD_TILE
        for k in range(1, len(sizes)):
            n, p = sizes[k][axis], sizes[k - 1][axis]
            if n > p:
                return False
            side = min(n, side * n // p + 3)
            if side > FOLD_REGION:
                return False
    return len(sizes) >= 2


@functools.lru_cache(maxsize=None)
def fold_footprint_sides(ns):
    """ns: one axis of a pyramid's sizes.  -> the largest footprint side per level k >= 1 over all tile positions, the footprint of
    [t0, t1] in the next level being [tap(t0).lo, tap(t1).hi] from the tap table"""
    t0 = np.arange(0, ns[0], FOLD_TILE)
    t1 = np.minimum(t0 + FOLD_TILE, ns[0]) - 1
    sides = []
    for k in range(1, len(ns)):
        lo, hi, _ = axis_table(ns[k], ns[k - 1])
        t0, t1 = lo[t0], hi[t1]
        assert (t0 <= t1).all() and t0.min() >= 0 and t1.max() < ns[k]
        sides.append(int((t1 - t0 + 1).max()))
    return sides


def adjoint_pair_ok(a, b):
    """the entry point's rule for two adjoint levels in one launch: each level halves the one above it to within a pixel"""
    return b >= 1 and 2 * b - 1 <= a <= 2 * b + 1


def adjoint_groups(sizes):
    """how strotss_fold_pyramid_adjoint walks the levels: [(k, 2)] where levels k, k+1, k+2 take one launch, [(k, 1)] otherwise"""
    out, k = [], 0
    while k + 1 < len(sizes):
        pair = k + 2 < len(sizes) and all(adjoint_pair_ok(sizes[k + j][ax], sizes[k + j + 1][ax]) for j in (0, 1) for ax in (0, 1))
        out.append((k, 2 if pair else 1))
        k += 2 if pair else 1
    return out


def contributors(in_size, out_size):
    """per input index i the first and last output index with a tap on i (first > last: none), from the tap table"""
    lo, hi, _ = axis_table(in_size, out_size)
    first = np.full(in_size, out_size, np.int64)
    last = np.full(in_size, -1, np.int64)
    o = np.arange(out_size)
    for t in (lo, hi):
        np.minimum.at(first, t, o)
        np.maximum.at(last, t, o)
    return first, last


def candidate_window(in_size, out_size):
    """the adjoint kernels' candidate outputs of every input index i: o in [floor((i - 0.5) / s - 0.5) - 1, ceil((i + 1.5) / s -
    0.5) + 1] clipped, s = fl32(in) / fl32(out), in float32.  The compiler may or may not contract the product and the
    subtraction, so both roundings are evaluated: -> (o0, o1) of the NARROWER window (what must still hold every contributor)
    and (o0, o1) of the WIDER one (what must still fit the LDS region)."""
    s = np.float32(in_size) / np.float32(out_size)
    inv = np.float32(1.0) / s
    i = np.arange(in_size, dtype=np.float32)
    res = []
    for shift, rnd, edge in ((np.float32(-0.5), np.floor, -1), (np.float32(1.5), np.ceil, 1)):
        a = i + shift
        plain = ((a * inv).astype(np.float32) - np.float32(0.5)).astype(np.float32)
        fused = (a.astype(np.float64) * np.float64(inv) - 0.5).astype(np.float32)
        res.append((rnd(plain).astype(np.int64) + edge, rnd(fused).astype(np.int64) + edge))
    (a0, b0), (a1, b1) = res
    clip0 = lambda v: np.maximum(v, 0)
    clip1 = lambda v: np.minimum(v, out_size - 1)
    return (clip0(np.maximum(a0, b0)), clip1(np.minimum(a1, b1))), (clip0(np.minimum(a0, b0)), clip1(np.maximum(a1, b1)))


@functools.lru_cache(maxsize=None)
def adjoint_pair_region_sides(n0, n1, n2):
    """one axis of an adjoint pair (levels n0 -> n1 -> n2): over all workgroups, the largest side of the middle-level region
    a workgroup computes into LDS = its own 16-pixel tile of level 1 joined with what its 8-pixel tile of level 2 gathers from
    -> (by the tap table's true contributors, by the kernel's wider candidate window)"""
    groups = max(-(-n2 // ADJ2_T2), -(-n1 // (2 * ADJ2_T2)))
    j = np.arange(groups)
    o0, o1 = j * 2 * ADJ2_T2, np.minimum(j * 2 * ADJ2_T2 + 2 * ADJ2_T2, n1) - 1          # own tile of level 1 (empty: o0 > o1)
    o0 = np.where(o0 <= o1, o0, n1)
    starts = np.arange(0, n2, ADJ2_T2)
    best = []
    for f, l in (contributors(n2, n1), candidate_window(n2, n1)[1]):
        r0, r1 = o0.copy(), o1.copy()
        r0[:len(starts)] = np.minimum(r0[:len(starts)], np.minimum.reduceat(f, starts))
        r1[:len(starts)] = np.maximum(r1[:len(starts)], np.maximum.reduceat(l, starts))
        best.append(int((r1 - r0 + 1).max()))
    return tuple(best)


def fused_forms_fit(sizes):
    """whether no workgroup of the one-launch fold and of the adjoint's pair launches can leave its LDS region at this pyramid:
    every footprint side from the tap table within 24 (fold) and every middle-level region within 32 (adjoint pairs, by the
    kernel's widest candidate window), wherever the entry points take the fused kernels.  tests/test_hip_pixel_path.py launches
    the fused forms only at pyramids for which this holds."""
    ok = True
    if host_admits_fold(sizes):
        ok = all(s <= FOLD_REGION for ax in (0, 1) for s in fold_footprint_sides(tuple(hw[ax] for hw in sizes)))
    for k, n in adjoint_groups(sizes):
        if n == 2:
            ok = ok and all(max(adjoint_pair_region_sides(*(sizes[k + q][ax] for q in range(3)))) <= ADJ2_REGION for ax in (0, 1))
    return ok


# ------------------------------------------------------------------ first layer
def preprocess_constants():
    """(mean, fl32(1 / std)) as the kernel receives them: float32 mean, float32 reciprocal of the float32 std"""
    mean = np.float32(O.IMAGENET_MEAN)
    return mean, (np.float32(1.0) / np.float32(O.IMAGENET_STD)).astype(np.float32)


def first_layer_weights(cout=64):
    """(w (27, cout), bias (cout)) float32 from the oracle's synthetic VGG: the first cout channels of block1_conv1"""
    w, b = O.make_synthetic_vgg16_weights(0)[0]
    return w.numpy().reshape(27, 64)[:, :cout].copy(), b.numpy()[:cout].copy()


def first_layer(img, w, b, rows=None):
    """img (h, w, 3) float32 -> (pre-activation in float64, bound) for the image rows `rows` = (r0, r1) (default: all):
    27 taps of the zero-padded preprocessed image, k = (dy * 3 + dx) * 3 + ci"""
    mean, istd = preprocess_constants()
    h, wd = img.shape[:2]
    r0, r1 = rows or (0, h)
    p = np.zeros((h + 2, wd + 2, 3))
    p[1:-1, 1:-1] = (img.astype(np.float64) - mean.astype(np.float64)) * istd.astype(np.float64)
    taps = np.concatenate([p[r0 + dy:r1 + dy, dx:dx + wd] for dy in range(3) for dx in range(3)], axis=2)     # (rows, w, 27)
    w64, b64 = np.asarray(w, np.float64), np.asarray(b, np.float64)
    pre = taps @ w64 + b64
    bound = FIRST_LAYER_K * U * (np.abs(taps) @ np.abs(w64) + np.abs(b64))
    return pre, bound


def flipped_weights(w):
    """w (27, cout) -> w_tic (9, 3, cout): the spatially flipped kernel, tap' = (2 - dy) * 3 + (2 - dx)"""
    cout = w.shape[1]
    return np.ascontiguousarray(w.reshape(3, 3, 3, cout)[::-1, ::-1]).reshape(9, 3, cout)


def first_layer_dgrad(gout, w):
    """gout (h, w, cout) float32, w (27, cout) -> (gimg (h, w, 3) in float64, B): gimg[y, x, ci] = fl32(1 / std[ci]) *
    sum_{dy, dx, co} gout[y - dy + 1, x - dx + 1, co] w[(dy, dx, ci), co]"""
    _, istd = preprocess_constants()
    h, wd, cout = gout.shape
    g = np.zeros((h + 2, wd + 2, cout))
    g[1:-1, 1:-1] = gout
    w4 = np.asarray(w, np.float64).reshape(3, 3, 3, cout)
    ref, b = np.zeros((h, wd, 3)), np.zeros((h, wd, 3))
    for dy in range(3):
        for dx in range(3):
            sl = g[2 - dy:2 - dy + h, 2 - dx:2 - dx + wd]
            ref += sl @ w4[dy, dx].T
            b += np.abs(sl) @ np.abs(w4[dy, dx]).T
    return ref * istd.astype(np.float64), b * istd.astype(np.float64)


def unpack_sign_words(words, h, w):
    """relu_bits (tiles, c) int32 -> bool (h, w, c): word (ty * TW + tx, ch), byte r, bit q = act[4 ty + r, 4 tx + q, ch] > 0"""
    th, tw = (h + 3) // 4, (w + 3) // 4
    wd = np.asarray(words).astype(np.int64) & 0xFFFFFFFF
    c = wd.shape[1]
    wd = wd.reshape(th, tw, c)
    out = np.zeros((th * 4, tw * 4, c), dtype=bool)
    for r in range(4):
        for q in range(4):
            out[r::4, q::4] = (wd >> (8 * r + q)) & 1
    return out[:h, :w]


# ------------------------------------------------------------------ max-pool
def windows(x):
    """x (h, w, c) -> (4, h // 2, w // 2, c): the window positions in scan order (0,0), (0,1), (1,0), (1,1)"""
    ho, wo = x.shape[0] // 2, x.shape[1] // 2
    return np.stack([x[dy:2 * ho:2, dx:2 * wo:2] for dy in (0, 1) for dx in (0, 1)])


def maxpool(x):
    """-> (pooled values, codes): the index of the FIRST maximum in scan order, 4 where that maximum is not positive"""
    v = windows(x)
    best = np.argmax(v, axis=0)                       # numpy: the first occurrence
    mx = v.max(axis=0)
    return mx, np.where(mx > 0, best, 4).astype(np.uint8)


def maxpool_bwd(code, gout, h, w):
    """gin (h, w, c): gout routed to the coded position, +0.0 elsewhere (an odd last row and column included)"""
    ho, wo = h // 2, w // 2
    gin = np.zeros((h, w, gout.shape[2]), np.float32)
    for q in range(4):
        gin[q >> 1:2 * ho:2, q & 1:2 * wo:2] = np.where(code == q, gout, np.float32(0))
    return gin


# ------------------------------------------------------------------ rmsprop
def rmsprop(var, rms, g, lr, rho, eps):
    """one step from the float32 state (var, rms) and gradient g, in float64 on the float32 values of lr, rho, eps
    -> (rms', bound, var', bound)"""
    lr, rho, eps = (float(np.float32(v)) for v in (lr, rho, eps))
    var, rms, g = (np.asarray(a, np.float64) for a in (var, rms, g))
    r = rho * rms + (1.0 - rho) * g * g
    delta = lr * g / (np.sqrt(r) + eps)
    v = var - delta
    return r, 3 * U * r, v, 6 * U * np.abs(delta) + U * np.abs(v)
