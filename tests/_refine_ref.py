"""Float64 NumPy restatement of the mask refinement behind --refine_masks: the cell colours, the joint
bilateral votes of every pixel among the cells around its own, the chosen label with the winning vote and the runner-up, the
pixel counts; the error bound E of the votes and the test data.  Pure host code: the CPU tests check it against itself, the
GPU tests check the kernels against it."""
import numpy as np

U24 = 2.0 ** -24
RADIUS, SIGMA_S, SIGMA_R = 2, 1.0, 0.1            # the product's constants (nn.strotss_utils.REFINE_*)
SIGMA_RANGE = (0.01, 1.0)


def vote_eps(sigma_r: float) -> float:
    """The relative error eps of one vote, for colours in [0, 1].

    The kernel and this file differ in three ways.  (1) The kernel's cell colour is the float32 rounding of a float64 mean:
    |dm| <= (2^-24 + 2^-33) |m| per cell (2^-33 covers the float64 summation of a cell of up to 2^20 pixels), |m| <= sqrt 3 and
    |I - m| <= sqrt 3, so |I - m|^2 moves by at most 2 |I - m| |dm| + |dm|^2 <= 6 (2^-24 + 2^-33) and the colour exponent
    |I - m|^2 / (2 sigma_r^2) by at most d = 3 (2^-24 + 2^-33) / sigma_r^2: a weight changes by a factor within exp(+-d).
    (2) Each side evaluates the exponent in float64 with a handful of roundings (relative 8 x 2^-53 of an exponent that is
    below 745 for any weight that does not underflow: 7e-13 absolute in the exponent) and an `exp` good to a few ulp
    (2^-51); this file multiplies two exponentials where the kernel takes one of the summed exponent (two more ulp).
    (3) At most 81 float64 additions (radius 4; 25 at the product's radius 2): 81 x 2^-53.  (2) and (3) together stay below
    2^-39 = 1.8e-12.  Every weight is positive, so a vote -- a sum of weights -- has the relative error of its weights:
        eps = expm1(3 (2^-24 + 2^-33) / sigma_r^2) + 2^-39        (1.8e-7 at sigma_r = 1, 1.8e-5 at 0.1, 1.8e-3 at 0.01)"""
    return float(np.expm1(3.0 * (U24 + 2.0 ** -33) / sigma_r ** 2) + 2.0 ** -39)


def bound(best, sigma_r: float):
    """E, relative to the winning vote: every vote is at most `best`, so each is known to eps best and two of them compare
    wrongly only when they are within E = 2 eps best of each other.  The 1e-300 covers votes that underflow: below the
    normal range of float64 a weight has no relative accuracy, on either side."""
    return 2.0 * vote_eps(sigma_r) * np.maximum(best, 0.0) + 1e-300


def cell_index(n: int, g: int) -> np.ndarray:
    """(n,): the cell min(y g // n, g - 1) of every pixel row (column) -- what upsample_labels maps it to"""
    return np.minimum(np.arange(n) * g // n, g - 1)


def cell_means(img: np.ndarray, gh: int, gw: int) -> np.ndarray:
    """(gh, gw, 3) float64: the mean of the image over every cell's own pixels"""
    H, W = img.shape[:2]
    rows, cols = cell_index(H, gh), cell_index(W, gw)
    flat = (rows[:, None] * gw + cols[None, :]).reshape(-1)
    n = np.bincount(flat, minlength=gh * gw).astype(np.float64)
    x = img.astype(np.float64).reshape(-1, 3)
    sums = np.stack([np.bincount(flat, weights=x[:, c], minlength=gh * gw) for c in range(3)], axis=-1)
    return (sums / n[:, None]).reshape(gh, gw, 3)


def votes(img, grid, k: int, radius: int = RADIUS, sigma_s: float = SIGMA_S, sigma_r: float = SIGMA_R, means=None):
    """(vote (H, W, k) float64, present (H, W, k) bool): the votes of every pixel and which labels occur in its window.
    Cells with a label outside 0..k-1 are skipped.  means: the cell colours to use (default: cell_means in float64)."""
    H, W = img.shape[:2]
    gh, gw = grid.shape
    assert gh <= H and gw <= W
    m = cell_means(img, gh, gw) if means is None else np.asarray(means, dtype=np.float64)
    x = img.astype(np.float64)
    u = (np.arange(H) + 0.5) * gh / H - 0.5
    v = (np.arange(W) + 0.5) * gw / W - 0.5
    i0, j0 = cell_index(H, gh), cell_index(W, gw)
    vote = np.zeros((H, W, k))
    present = np.zeros((H, W, k), dtype=bool)
    for di in range(-radius, radius + 1):
        i = i0 + di
        for dj in range(-radius, radius + 1):
            j = j0 + dj
            ok = ((i >= 0) & (i < gh))[:, None] & ((j >= 0) & (j < gw))[None, :]
            ic, jc = np.clip(i, 0, gh - 1), np.clip(j, 0, gw - 1)
            d2 = ((u - i) ** 2)[:, None] + ((v - j) ** 2)[None, :]
            c2 = ((x - m[ic][:, jc]) ** 2).sum(axis=-1)
            w = np.exp(-d2 / (2 * sigma_s ** 2)) * np.exp(-c2 / (2 * sigma_r ** 2))
            lab = grid[ic][:, jc]
            for l in range(k):
                hit = ok & (lab == l)
                vote[..., l] += np.where(hit, w, 0.0)
                present[..., l] |= hit
    return vote, present


def resolve(vote, present):
    """(label int32, best, second): the first arg-max among the labels present, its vote and the largest of the other present
    labels' votes (-inf when there is none); a window without any label in 0..k-1: label 0, best = second = -inf"""
    masked = np.where(present, vote, -np.inf)
    label = np.argmax(masked, axis=-1).astype(np.int32)                # the first of equal values
    best = np.take_along_axis(masked, label[..., None].astype(np.int64), axis=-1)[..., 0]
    rest = masked.copy()
    np.put_along_axis(rest, label[..., None].astype(np.int64), -np.inf, axis=-1)
    second = rest.max(axis=-1)
    return label, best, second


def refine(img, grid, k, radius=RADIUS, sigma_s=SIGMA_S, sigma_r=SIGMA_R):
    """dict(label (H, W) int32, best, second, count (k,), vote, present, means)"""
    means = cell_means(img, *grid.shape)
    vote, present = votes(img, grid, k, radius, sigma_s, sigma_r, means)
    label, best, second = resolve(vote, present)
    return dict(label=label, best=best, second=second, count=np.bincount(label.reshape(-1), minlength=k)[:k], vote=vote,
                present=present, means=means)


def admissible(label, vote, present, best, sigma_r) -> np.ndarray:
    """per pixel: `label` occurs in the window and its float64 vote is within E of the best vote"""
    idx = label[..., None].astype(np.int64)
    mine = np.take_along_axis(vote, idx, axis=-1)[..., 0]
    here = np.take_along_axis(present, idx, axis=-1)[..., 0]
    return here & (mine >= best - bound(best, sigma_r))


def upsample_labels(grid: np.ndarray, H: int, W: int) -> np.ndarray:
    gh, gw = grid.shape
    return grid[cell_index(H, gh)][:, cell_index(W, gw)]


# ------------------------------------------------------------------ test data
PALETTE = np.array([(r, g, b) for r in (0.1, 0.5, 0.9) for g in (0.1, 0.5, 0.9) for b in (0.1, 0.5, 0.9)])[
    [0, 26, 2, 24, 6, 20, 8, 18, 13, 4, 22, 10, 16, 12, 14, 1]]       # 16 colours, pairwise at least 0.4 apart


def planted_image(H: int, W: int, gh: int, gw: int, k: int, seed: int, noise: float = 0.02):
    """(image (H, W, 3) float32 in [0, 1], grid (gh, gw) int32, pixel labels (H, W)): the image is cut into the Voronoi regions
    of k random points, region l painted PALETTE[l] plus uniform noise of +-`noise`; a cell takes the label of the pixel at its
    centre.  The region borders run through the cells, not along them."""
    rng = np.random.default_rng(seed)
    pts = rng.random((k, 2))
    yy, xx = (np.arange(H) + 0.5) / H, (np.arange(W) + 0.5) / W
    d = (yy[:, None, None] - pts[None, None, :, 0]) ** 2 + (xx[None, :, None] - pts[None, None, :, 1]) ** 2
    pixel = np.argmin(d, axis=-1).astype(np.int32)
    img = (PALETTE[pixel] + rng.uniform(-noise, noise, size=(H, W, 3))).astype(np.float32)
    cy = np.minimum(((np.arange(gh) + 0.5) * H / gh).astype(np.int64), H - 1)
    cx = np.minimum(((np.arange(gw) + 0.5) * W / gw).astype(np.int64), W - 1)
    return img, np.ascontiguousarray(pixel[cy][:, cx]), pixel


def noise_image(H: int, W: int, gh: int, gw: int, k: int, seed: int):
    """the unstructured case: a uniform-noise image with uniformly random labels"""
    rng = np.random.default_rng(seed)
    return rng.random((H, W, 3)).astype(np.float32), rng.integers(0, k, size=(gh, gw)).astype(np.int32)


# (H, W, gh, gw, k): one pixel; one pixel per cell and a window wider than the grid in x; sizes that do not divide; the
# largest k; tile tails in both directions; the product's shape
SHAPES = [(1, 1, 1, 1, 1), (7, 5, 7, 5, 2), (33, 47, 5, 7, 3), (64, 96, 16, 24, 16), (300, 257, 64, 55, 5),
          (1024, 683, 64, 43, 8)]
# (shape, radius, sigma_r): every shape at the product's constants, one at the two other radii, one at both ends of sigma_r
CASES = [(s, RADIUS, SIGMA_R) for s in SHAPES] + [(SHAPES[2], 1, SIGMA_R), (SHAPES[2], 4, SIGMA_R),
                                                  (SHAPES[3], RADIUS, SIGMA_RANGE[0]), (SHAPES[3], RADIUS, SIGMA_RANGE[1])]
UNSTRUCTURED = ((96, 128, 24, 32, 5), RADIUS, SIGMA_R)
_SEED = 18
_results = {}


def case_id(case) -> str:
    (H, W, gh, gw, k), radius, sigma_r = case
    return f"{H}x{W}-grid{gh}x{gw}-k{k}-R{radius}-s{sigma_r:g}"


def case_data(case):
    """(image, grid) of a case"""
    shape = case[0]
    if case == UNSTRUCTURED:
        return noise_image(*shape, seed=_SEED)
    return planted_image(*shape, seed=_SEED + sum(shape))[:2]


def case_result(case):
    """(image, grid, refine(...)) of a case, computed once per process and left unchanged"""
    if case not in _results:
        img, grid = case_data(case)
        _results[case] = (img, grid, refine(img, grid, case[0][4], case[1], SIGMA_S, case[2]))
    return _results[case]
