"""Float64 NumPy restatement of the region clustering behind --auto_masks: the assignment and the
centre update of spherical k-means, the deterministic farthest-first initialisation, the loop of nn.strotss_utils
.spherical_kmeans and the nearest-neighbour upsampling of a label grid to masks; the error bound of the assignment and the
planted test data.  Pure host code: the CPU tests check it against itself, the GPU tests check the kernels against it."""
import numpy as np

U24 = 2.0 ** -24
ITERS = 16


def pad32(v: int) -> int:
    return (v + 31) // 32 * 32


def gamma32(m: int) -> float:
    """the float32 summation constant gamma_m = m u / (1 - m u), u = 2^-24 (Higham, Accuracy and Stability, section 3.1)"""
    return m * U24 / (1.0 - m * U24)


def assign_bound(d: int) -> float:
    """E = 2 gamma_{d+2}: a float32 dot product of length d, times inv_norm, is within gamma_{d+2} |x| |c| / |x| of the exact
    cosine, so two cosines computed that way compare wrongly only when they are within E of each other (|c| = 1)"""
    return 2.0 * gamma32(d + 2)


def planted_rows(n: int, d: int, k: int, noise: float, seed: int, scale: float = 2.0):
    """(x, planted labels): non-negative rows max(P[lab] + noise N(0, 1), 0) as float32, P k random non-negative prototypes
    (exponential with mean `scale`; scale 0: pure noise), lab uniform in 0..k-1 with every label present when n >= k,
    zero-padded to (pad32(n), pad32(d))"""
    rng = np.random.default_rng(seed)
    P = rng.exponential(scale, size=(k, d)) if scale > 0 else np.zeros((k, d))
    lab = rng.integers(0, k, size=n)
    lab[:min(n, k)] = np.arange(min(n, k))
    rows = np.maximum(P[lab] + noise * rng.standard_normal((n, d)), 0.0).astype(np.float32)
    x = np.zeros((pad32(n), pad32(d)), dtype=np.float32)
    x[:n, :d] = rows
    return x, lab.astype(np.int32)


def inv_norm(x: np.ndarray, n: int) -> np.ndarray:
    """strotss_row_inv_norm: 1 / sqrt(max(|x_i|^2, 1e-12)) rounded to float32, (rows,) with zeros beyond n"""
    r = np.zeros(x.shape[0], dtype=np.float32)
    r[:n] = (1.0 / np.sqrt(np.maximum((x[:n].astype(np.float64) ** 2).sum(1), 1e-12))).astype(np.float32)
    return r


def scores(x, inv, n, d, centres) -> np.ndarray:
    """(n, k) float64: (x_i . c_j) inv_i"""
    c = np.asarray(centres, dtype=np.float64)[:, :d]
    return (x[:n, :d].astype(np.float64) @ c.T) * inv[:n].astype(np.float64)[:, None]


def assign(x, inv, n, d, centres):
    """(label int32, best, second, scores): the first arg-max per row, its value, the largest of the others (-inf for one
    centre); a row with inv == 0 gets label 0 and best = second = 0"""
    s = scores(x, inv, n, d, centres)
    label = np.argmax(s, axis=1).astype(np.int32)                   # the first of equal values
    best = s[np.arange(n), label]
    rest = s.copy()
    rest[np.arange(n), label] = -np.inf
    second = rest.max(axis=1) if s.shape[1] > 1 else np.full(n, -np.inf)
    zero = inv[:n] == 0
    label[zero], best[zero], second[zero] = 0, 0.0, 0.0
    return label, best, second, s


def update(x, inv, label, n, d, k, centres):
    """(centres (k, d) float64, count (k,) int64): centre j = the normalised sum of x_i inv_i over the rows with label j; an
    empty cluster keeps its centre; labels outside 0..k-1 are skipped"""
    u = x[:n, :d].astype(np.float64) * inv[:n].astype(np.float64)[:, None]
    out = np.array(np.asarray(centres, dtype=np.float64)[:k, :d])
    count = np.zeros(k, dtype=np.int64)
    for j in range(k):
        rows = label[:n] == j
        count[j] = int(rows.sum())
        if count[j]:
            s = u[rows].sum(axis=0)
            norm = np.sqrt((s * s).sum())
            out[j] = s / norm if norm > 0 else 0.0
    return out, count


def farthest_first(x, inv, n, d, k):
    """(centres (k, d) float64, chosen rows): centre 0 = the unit row with the largest cosine to the normalised sum of all
    unit rows, centre j = the unit row whose largest cosine to centres 0..j-1 is smallest; the lowest row index on ties"""
    u = x[:n, :d].astype(np.float64) * inv[:n].astype(np.float64)[:, None]
    mean = u.sum(axis=0)
    mean /= max(np.sqrt((mean * mean).sum()), 1e-300)
    chosen = [int(np.argmax(u @ mean))]
    nearest = u @ u[chosen[0]]
    for _ in range(1, k):
        chosen.append(int(np.argmin(nearest)))
        nearest = np.maximum(nearest, u @ u[chosen[-1]])
    return u[chosen].copy(), chosen


def spherical_kmeans(x, n, d, k, iters=ITERS, inv=None):
    """The loop of nn.strotss_utils.spherical_kmeans: farthest-first centres, one assignment, then `iters` times (update,
    assign).  -> dict(label, centres (k, d), count, objective [iters], margins [iters + 1] of best - second per row)"""
    inv = inv_norm(x, n) if inv is None else inv
    centres, _ = farthest_first(x, inv, n, d, k)
    label, best, second, _ = assign(x, inv, n, d, centres)
    objective, margins = [], [best - second]
    for _ in range(iters):
        centres, _ = update(x, inv, label, n, d, k, centres)
        label, best, second, _ = assign(x, inv, n, d, centres)
        objective.append(float(best.mean()))
        margins.append(best - second)
    return dict(label=label, centres=centres, count=np.bincount(label, minlength=k), objective=objective, margins=margins)


def admissible(label, s, bound: float) -> np.ndarray:
    """per row: the score of `label` is within `bound` of the row's largest float64 score"""
    return s[np.arange(s.shape[0]), label] >= s.max(axis=1) - bound


def grid_points(h: int, w: int, cells: int = 64):
    """(rows, columns) of the regular grid of an (h, w) image: stride g = ceil(long side / cells), from g // 2"""
    g = -(-max(h, w) // cells)
    return np.arange(g // 2, h, g), np.arange(g // 2, w, g)


def upsample_labels(grid: np.ndarray, H: int, W: int) -> np.ndarray:
    """(H, W): pixel (y, x) takes grid cell (min(y gh // H, gh - 1), min(x gw // W, gw - 1))"""
    gh, gw = grid.shape
    ys = np.minimum(np.arange(H) * gh // H, gh - 1)
    xs = np.minimum(np.arange(W) * gw // W, gw - 1)
    return grid[ys][:, xs]


def masks_from_labels(labels: np.ndarray, k: int):
    """k (H, W, 1) float32 0/1 masks, one per label in ascending order: a partition of the image"""
    return [(labels == j).astype(np.float32)[..., None] for j in range(k)]


CORNER_COLOURS = [(r, g, b) for r in (0, 255) for g in (0, 255) for b in (0, 255)]     # ascending (r, g, b)


def same_partition(a, b, k: int) -> bool:
    """the two labelings are equal up to a permutation of the k labels"""
    table = np.zeros((k, k), dtype=np.int64)
    np.add.at(table, (np.asarray(a), np.asarray(b)), 1)
    return bool(((table > 0).sum(axis=0) == 1).all() and ((table > 0).sum(axis=1) == 1).all())


# The k-means cases of the tests, arguments of planted_rows: (n, d, k, noise, seed[, scale]).  PLANTED: noise 1.0 around
# prototypes of mean 2 -- every margin of every iteration is far above E (test_cluster_cpu.py), so labels compare exactly.
# UNSTRUCTURED: a narrow case and pure noise (scale 0): margins down to 1e-9, compared through admissibility.
PLANTED = [(2048, 2179, 2, 1.0, 102), (2048, 2179, 5, 1.0, 105), (2048, 2179, 16, 1.0, 116)]
UNSTRUCTURED = [(1000, 35, 16, 1.0, 7), (4096, 2179, 16, 1.0, 9, 0.0)]
_results = {}


def planted_result(case):
    """spherical_kmeans of planted_rows(*case), computed once per process"""
    if case not in _results:
        x, _ = planted_rows(*case)
        _results[case] = spherical_kmeans(x, case[0], case[1], case[2])
    return _results[case]
