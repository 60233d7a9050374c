"""The detail map of --sample_map auto (include/strotss_hip.h: strotss_detail_map) in NumPy: the
statement in float64 (detail_map_ref) and its float32 twin (detail_map_f32: the same formulas with float32 luma, gradient,
division and square root, every operation rounded on its own, and float64 sums), plus the shapes and parameters the CPU and
GPU tests share.  Both take gain and floor at their float32 values, as the C entry receives them.

Window sums are DIRECT sums in ascending index order, the column pass (over y) first, then the row pass (over x): a region
whose gradient energy is zero sums to zero exactly, which running sums would not guarantee."""
import numpy as np

LUMA = (0.299, 0.587, 0.114)
MAX_RADIUS = 64


def _clamped_diff(y, axis):
    """(y[i + 1] - y[i - 1]) with both indices clamped to the axis, in y's dtype; a 1-element axis gives 0"""
    n = y.shape[axis]
    idx = np.arange(n)
    return np.take(y, np.minimum(idx + 1, n - 1), axis=axis) - np.take(y, np.maximum(idx - 1, 0), axis=axis)


def _box_sum(a, r, axis):
    """sum of float64 `a` over [i - r, i + r] clipped to the axis, ascending index order"""
    a = np.moveaxis(a, axis, 0)
    n = a.shape[0]
    out = np.zeros_like(a)
    for d in range(-r, r + 1):
        lo, hi = max(0, -d), min(n, n - d)
        if lo < hi:
            out[lo:hi] += a[lo + d:hi + d]
    return np.moveaxis(out, 0, axis)


def window_counts(h, w, r):
    """(h, w) number of pixels inside the clipped (2r+1) x (2r+1) window"""
    ys, xs = np.arange(h), np.arange(w)
    ny = np.minimum(ys + r, h - 1) - np.maximum(ys - r, 0) + 1
    nx = np.minimum(xs + r, w - 1) - np.maximum(xs - r, 0) + 1
    return ny[:, None] * nx[None, :]


def energy(img, dtype):
    """gradient energy e = gx^2 + gy^2 of the luma, every operation in `dtype`"""
    img = np.asarray(img, dtype=dtype)
    k = [dtype(c) for c in LUMA]
    y = (k[0] * img[..., 0] + k[1] * img[..., 1]) + k[2] * img[..., 2]
    gx, gy = _clamped_diff(y, 1) * dtype(0.5), _clamped_diff(y, 0) * dtype(0.5)
    return gx * gx + gy * gy


def local_detail(img, r, dtype=np.float64):
    """s (h, w) in `dtype`: the root of the windowed mean of e, the window sums in float64"""
    e = energy(img, dtype)
    h, w = e.shape
    sums = _box_sum(_box_sum(e.astype(np.float64), r, 0), r, 1)
    n = window_counts(h, w, r)
    return np.sqrt(sums.astype(dtype) / n.astype(dtype))


def _check(r, gain, floor):
    assert 1 <= int(r) <= MAX_RADIUS and np.isfinite(gain) and gain > 0 and np.isfinite(floor) and 0 <= floor <= 1


def detail_map_ref(img, r, gain=2.0, floor=0.25):
    """the statement in float64 -> (h, w) float64"""
    _check(r, gain, floor)
    g, f = float(np.float32(gain)), float(np.float32(floor))
    s = local_detail(img, int(r), np.float64)
    m = s.sum() / s.size
    if m == 0:
        return np.ones_like(s)
    return f + (1.0 - f) * np.minimum(1.0, s / (g * m))


def detail_map_f32(img, r, gain=2.0, floor=0.25):
    """the float32 twin -> (h, w) float32; where the minimum is 1 the result is 1 itself"""
    _check(r, gain, floor)
    g, f = np.float32(gain), np.float32(floor)
    s = local_detail(img, int(r), np.float32)
    m = s.astype(np.float64).sum() / s.size
    denom = g * np.float32(m)
    if denom == 0:
        return np.ones_like(s)
    with np.errstate(over="ignore"):
        t = s / denom
    return np.where(t >= 1, np.float32(1), f + (np.float32(1) - f) * t).astype(np.float32)


# ------------------------------------------------------------------ the cases of the GPU test
# The kernels' tiles (csrc/detail_map.hip): the column pass works on 64 x 16 pixel tiles (DM_COLS_X x DM_COLS_Y), the row
# pass on 256 pixels of one row (DM_ROW_THREADS), the scale pass on float4 groups with a scalar tail.
COLS_TILE_X, COLS_TILE_Y, ROW_TILE = 64, 16, 256
BIG = (2 * COLS_TILE_Y * 4 + 22, ROW_TILE + 37, 64)      # (150, 293): 9 tile rows + 6, one row tile + 37, 4 column tiles + 37
assert BIG[0] % COLS_TILE_Y and BIG[1] % COLS_TILE_X and BIG[1] % ROW_TILE and BIG[0] > COLS_TILE_Y and BIG[1] > ROW_TILE
SHAPES = [(1, 1, 1), (1, 9, 2), (9, 1, 2), (5, 7, 8), (33, 65, 1), (33, 65, 4), BIG]
# (gain, floor): the defaults; a gain small enough that min(1, .) acts, with floor 0; floor 1 (all ones)
PARAMS = [(2.0, 0.25), (0.25, 0.0), (2.0, 1.0)]
KINDS = ("random", "edge")


def image(kind, h, w):
    """(h, w, 3) float32 in [0, 1]: uniform noise, or a slanted step edge between two colours"""
    if kind == "random":
        return np.random.default_rng(1000 * h + w).random((h, w, 3), dtype=np.float32)
    ys, xs = np.mgrid[0:h, 0:w]
    right = (2 * xs + ys) > (w + h // 2)
    img = np.empty((h, w, 3), dtype=np.float32)
    img[...] = np.float32([0.2, 0.3, 0.1])
    img[right] = np.float32([0.9, 0.6, 0.8])
    return img


_cache = {}


def case(kind, shape, params):
    """(img, float64 reference, float32 twin, E32 = max |twin - reference|) of a case, computed once"""
    key = (kind, tuple(shape), tuple(params))
    if key not in _cache:
        h, w, r = shape
        img = image(kind, h, w)
        ref = detail_map_ref(img, r, *params)
        twin = detail_map_f32(img, r, *params)
        _cache[key] = (img, ref, twin, float(np.abs(twin.astype(np.float64) - ref).max()))
    return _cache[key]
