"""The cases, comparisons and NumPy stand-ins of the mask kernels' edge tests ("Mask kernel edges"):
strotss_refine_labels at the sizes where its LDS staging takes a second and third trip, fills its footprint array and walks more
tiles and cells than a launch has workgroups and waves; the k-means assignment at every 256-column half, 512-column chunk and
KP edge; the centre update at its column-block and row-block edges; the label warp at a ragged last workgroup and on the first
source pixel inside and outside each border.  The references are tests/_refine_ref.py, _cluster_ref.py and _track_ref.py as they
stand; this file holds what the CPU file (tests/test_mask_edges_cpu.py) and the GPU file (tests/test_hip_mask_edges.py) share:
the data of every case, ONE comparison per kernel that returns figures and the list of checks they miss, and stand-ins that
compute what a kernel with a planted error would.  Pure host code."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as KR  # noqa: E402
import _refine_ref as R  # noqa: E402
import _track_ref as TR  # noqa: E402

U23, U24 = 2.0 ** -23, 2.0 ** -24

# ------------------------------------------------------------------ 1. refinement
# the constants of csrc/refine.hip, restated
RF_THREADS, RF_TILE_W, RF_TILE_H, RF_MAX_RADIUS, RF_MAX_GRID, RF_CELLS_PER_BLOCK = 256, 32, 8, 4, 16384, 4
RF_FOOT_H, RF_FOOT_W = RF_TILE_H + 2 * RF_MAX_RADIUS, RF_TILE_W + 2 * RF_MAX_RADIUS          # 16, 40

# name -> ((h, w, gh, gw, k), radius, image, seed, claimed largest footprint (fh, fw), the edge it reaches).  sigma_s = radius
# / 2, so that the farthest cell of a window still carries exp(-4) of the nearest one's spatial weight: at the product's sigma_s
# = 1 the corner cells of a radius-4 window weigh exp(-16) = 1e-7 of a vote, below the bound of 3.6e-5, and a wrong quad
# staged there could not be seen.  sigma_r: the product's 0.1 on planted images (the cells of a pixel's own region weigh
# exp(-0.24) at least); 1.0, the upper end of its range, on noise images, where at 0.1 every cell but a pixel's own would weigh
# exp(-25) and the random labels around it would go unread.
REFINE_CASES = {
    "full-k16": ((24, 100, 24, 100, 16), 4, "planted", 1, (16, 40), "16 x 40 = 640 staged cells: the whole LDS array, three trips"),
    "full-k5": ((24, 100, 24, 100, 5), 4, "noise", 2, (16, 40), "the same footprint under KP = 8 and random labels"),
    "trip2-r2": ((24, 100, 24, 100, 8), 2, "planted", 3, (12, 36), "12 x 36 = 432 cells: a second trip at the product's radius"),
    "ragged-r4": ((37, 70, 36, 69, 4), 4, "planted", 4, (16, 40), "cells of 1 or 2 pixels: full footprint off the diagonal"),
    "ragged-r3": ((41, 131, 29, 97, 9), 3, "noise", 5, (12, 30), "5 to 6 cell rows per tile: fh changes from tile to tile, KP = 16"),
    "walks": ((131080, 3, 32771, 3, 3), 2, "planted", 6, (7, 3), "16385 tiles and 98313 cells: both persistent loops walk"),
}
AMBIGUOUS_CAP = 1e-3
LABEL_SENTINEL, COUNT_SENTINEL, VOTE_SENTINEL = -77, -55, -12345.0
_refine = {}


def sigma_s_of(radius: int) -> float:
    return radius / 2.0


def sigma_r_of(kind: str) -> float:
    return R.SIGMA_R if kind == "planted" else R.SIGMA_RANGE[1]


def axis_footprints(n: int, g: int, radius: int, tile: int):
    """[(first cell, cells)] of every tile along one axis, by the kernel's formula: the tile's own cells plus `radius` on each
    side, clipped to the grid"""
    out = []
    for t0 in range(0, n, tile):
        t1 = min(n, t0 + tile) - 1
        lo, hi = max(0, t0 * g // n - radius), min(g - 1, t1 * g // n + radius)
        out.append((lo, hi - lo + 1))
    return out


def footprints(h, w, gh, gw, radius):
    """(fh per tile row, fw per tile column): the footprint of tile (ty, tx) is fh[ty] x fw[tx]"""
    return ([f for _, f in axis_footprints(h, gh, radius, RF_TILE_H)], [f for _, f in axis_footprints(w, gw, radius, RF_TILE_W)])


def refine_counts(h, w, gh, gw):
    """(tiles, cells, workgroups of the vote launch, cells the mean launch takes in one pass)"""
    tiles = -(-h // RF_TILE_H) * -(-w // RF_TILE_W)
    blocks = min(-(-gh * gw // RF_CELLS_PER_BLOCK), RF_MAX_GRID)
    return tiles, gh * gw, min(tiles, RF_MAX_GRID), blocks * RF_CELLS_PER_BLOCK


def refine_case(name):
    """(img, grid, reference dict, (k, radius, sigma_s, sigma_r)), computed once and left unchanged"""
    if name not in _refine:
        (h, w, gh, gw, k), radius, kind, seed = REFINE_CASES[name][:4]
        if kind == "planted":
            img, grid = R.planted_image(h, w, gh, gw, k, seed)[:2]
        else:
            img, grid = R.noise_image(h, w, gh, gw, k, seed)
        sigma_r = sigma_r_of(kind)
        ref = R.refine(img, grid, k, radius, sigma_s_of(radius), sigma_r)
        _refine[name] = (img, grid, ref, (k, radius, sigma_s_of(radius), sigma_r))
    return _refine[name]


def ambiguous_share(ref, sigma_r) -> float:
    """the share of pixels at which `admissible` allows more than one label"""
    near = ref["present"] & (ref["vote"] >= (ref["best"] - R.bound(ref["best"], sigma_r))[..., None])
    return float((near.sum(axis=-1) > 1).mean())


def _worst(err, allowed) -> float:
    """the largest err / allowed; inf where either is not a number"""
    if err.size == 0:
        return 0.0
    ratio = err / allowed
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def refine_figures(got, ref, k, sigma_r):
    """got: dict(label (h, w) int32, best, second (h, w) float64, count (k,) int32, mean (gh, gw, 3) float32, guards {name:
    intact}) as read back from sentinel-filled outputs.  -> the figures the tests print, record and judge"""
    label, best, second = got["label"], got["best"], got["second"]
    inside = (label >= 0) & (label < k)
    ok = inside & R.admissible(np.where(inside, label, 0), ref["vote"], ref["present"], ref["best"], sigma_r)
    E = R.bound(ref["best"], sigma_r)
    both = np.isfinite(ref["second"])
    with np.errstate(invalid="ignore"):
        fig = dict(inadmissible=int((~ok).sum()), unwritten=int((label == LABEL_SENTINEL).sum()),
                   best=_worst(np.abs(best - ref["best"]), E), second=_worst(np.abs(second[both] - ref["second"][both]), E[both]),
                   second_inf=int((np.isneginf(second) != ~both).sum()))
    fig["count_ok"] = bool(np.array_equal(got["count"], np.bincount(label[inside].reshape(-1), minlength=k))
                           and int(got["count"].sum()) == label.size)
    fig["mean_bits"] = int((got["mean"].view(np.int32) != ref["means"].astype(np.float32).view(np.int32)).sum())
    fig["guards"] = [name for name, intact in got.get("guards", {}).items() if not intact]
    return fig


def refine_failures(fig):
    bad = []
    if fig["inadmissible"]:
        bad.append(f"{fig['inadmissible']} labels not admissible ({fig['unwritten']} pixels never written)")
    if not fig["best"] <= 1.0:
        bad.append(f"best off by {fig['best']:.3g} of its bound")
    if not fig["second"] <= 1.0 or fig["second_inf"]:
        bad.append(f"second off by {fig['second']:.3g} of its bound, {fig['second_inf']} -inf misplaced")
    if not fig["count_ok"]:
        bad.append("count is not the bincount of the labels")
    if fig["mean_bits"]:
        bad.append(f"{fig['mean_bits']} staged means differ in their bits")
    if fig["guards"]:
        bad.append(f"written outside the outputs: {fig['guards']}")
    return bad


def refine_standin(img, grid, k, radius, sigma_s, sigma_r, plant=None):
    """What refine_vote_kernel computes, tile by tile with ONE staging array that outlives the tiles (float32 means, float64
    votes), as dict(label, best, second, count, mean).  plant: None, "stage256" (the staging loop takes one trip: cells 256..
    keep what the tile before staged), "origin" (the footprint is staged from one cell row further down than it is read)."""
    h, w = img.shape[:2]
    gh, gw = grid.shape
    mean = R.cell_means(img, gh, gw).astype(np.float32)
    x = img.astype(np.float64)
    rgb, lab_s = np.zeros((RF_FOOT_H * RF_FOOT_W, 3)), np.zeros(RF_FOOT_H * RF_FOOT_W, dtype=np.int64)
    label = np.full((h, w), LABEL_SENTINEL, dtype=np.int32)
    best, second = np.full((h, w), VOTE_SENTINEL), np.full((h, w), VOTE_SENTINEL)
    inv2s, inv2r = 1.0 / (2.0 * sigma_s ** 2), 1.0 / (2.0 * sigma_r ** 2)
    rows, cols = axis_footprints(h, gh, radius, RF_TILE_H), axis_footprints(w, gw, radius, RF_TILE_W)
    for ty, (i_lo, fh) in enumerate(rows):
        for tx, (j_lo, fw) in enumerate(cols):
            assert fh * fw <= rgb.shape[0]
            c = np.arange(fh * fw)[:RF_THREADS if plant == "stage256" else None]
            gi = np.minimum(i_lo + c // fw + (plant == "origin"), gh - 1)
            rgb[c], lab_s[c] = mean[gi, j_lo + c % fw], grid[gi, j_lo + c % fw]
            ys, xs = np.arange(ty * RF_TILE_H, min(h, (ty + 1) * RF_TILE_H)), np.arange(tx * RF_TILE_W, min(w, (tx + 1) * RF_TILE_W))
            Y, X = (a.reshape(-1) for a in np.meshgrid(ys, xs, indexing="ij"))
            u, v = (Y + 0.5) * gh / h - 0.5, (X + 0.5) * gw / w - 0.5
            i0, j0 = Y * gh // h, X * gw // w
            vote, present = np.zeros((Y.size, k)), np.zeros((Y.size, k), dtype=bool)
            for di in range(-radius, radius + 1):
                for dj in range(-radius, radius + 1):
                    i, j = i0 + di, j0 + dj
                    ok = (i >= 0) & (i < gh) & (j >= 0) & (j < gw)
                    at = np.where(ok, (i - i_lo) * fw + (j - j_lo), 0)
                    c2 = ((x[Y, X] - rgb[at]) ** 2).sum(axis=-1)
                    wgt = np.exp(-(((u - i) ** 2 + (v - j) ** 2) * inv2s + c2 * inv2r))
                    for l in range(k):
                        hit = ok & (lab_s[at] == l)
                        vote[:, l] += np.where(hit, wgt, 0.0)
                        present[:, l] |= hit
            label[Y, X], best[Y, X], second[Y, X] = R.resolve(vote, present)
    return dict(label=label, best=best, second=second, mean=mean,
                count=np.bincount(label.reshape(-1), minlength=k)[:k].astype(np.int32))


def refine_walk_standin(img, grid, ref, k, plant=None):
    """The reference's own result as the outputs would hold it; plant "walk_stops": the tiles from RF_MAX_GRID on are never
    taken, their pixels keep the sentinels and are not counted"""
    h, w = img.shape[:2]
    label, best, second = ref["label"].copy(), ref["best"].copy(), ref["second"].copy()
    if plant == "walk_stops":
        tiles_x = -(-w // RF_TILE_W)
        tile = (np.arange(h)[:, None] // RF_TILE_H) * tiles_x + np.arange(w)[None, :] // RF_TILE_W
        label[tile >= RF_MAX_GRID], best[tile >= RF_MAX_GRID], second[tile >= RF_MAX_GRID] = LABEL_SENTINEL, VOTE_SENTINEL, VOTE_SENTINEL
    written = label[label != LABEL_SENTINEL]
    return dict(label=label, best=best, second=second, mean=ref["means"].astype(np.float32),
                count=np.bincount(written, minlength=k)[:k].astype(np.int32))


# ------------------------------------------------------------------ 2. assignment
ASSIGN_D = (252, 255, 256, 257, 260, 508, 512, 513, 516, 1024, 1027)
ASSIGN_K = (4, 5, 8, 9, 16)
ASSIGN_N = (31, 32, 33, 65)
ASSIGN_BETA = 0.05
ASSIGN_AMBIGUOUS_CAP = 1e-2
_assign = {}


def kp_of(k: int) -> int:
    return 4 if k <= 4 else 8 if k <= 8 else 16


def assign_data(d, k):
    """(x (96, ld), inv, c32 (k, ld), prior): 65 rows of _cluster_ref's generator, zero beyond d; the centres of the planted
    labels in float32, +inf in EVERY column beyond d -- x is zero there, so a finite value let through would add 0 and show
    nothing, where 0 x inf is a NaN in the score; priors uniform in -1..k.  The leading n rows are the case of n."""
    if (d, k) not in _assign:
        n = max(ASSIGN_N)
        x, planted = KR.planted_rows(n, d, k, 1.0, 3000 + d + k)
        inv = KR.inv_norm(x, n)
        centres, _ = KR.update(x, inv, planted, n, d, k, np.zeros((k, d)))
        c32 = np.full((k, x.shape[1]), np.inf, dtype=np.float32)
        c32[:, :d] = centres
        prior = np.random.default_rng(d + k).integers(-1, k + 1, size=x.shape[0]).astype(np.int32)
        _assign[(d, k)] = (x, inv, c32, prior)
    return _assign[(d, k)]


def assign_reference(x, inv, n, d, c32, prior=None, beta=0.0):
    """(label, best, second, score): _cluster_ref.assign, or _track_ref.assign_prior with its biased scores"""
    if prior is None:
        return KR.assign(x, inv, n, d, c32)
    label, best, second, _, score = TR.assign_prior(x, inv, n, d, c32, prior, beta)
    return label, best, second, score


def assign_margin(score) -> np.ndarray:
    return TR.biased_margin(score)


def assign_figures(got, ref, d):
    """got: (label, best, second) of the kernel, ref: assign_reference(...).  The tolerance of test_hip_cluster.py's
    test_assign_matches_float64: labels admissible within E = assign_bound(d) and equal where the margin is wider, best and
    second within E / 2 + 2^-23"""
    label, best, second = got
    ref_label, ref_best, ref_second, score = ref
    n, k = score.shape
    E = KR.assign_bound(d)
    tol = E / 2 + U23
    inside = (label >= 0) & (label < k)
    ok = inside & KR.admissible(np.where(inside, label, 0), score, E)
    wide = assign_margin(score) > E
    same = label == ref_label
    with np.errstate(invalid="ignore"):
        fig = dict(inadmissible=int((~ok).sum()), differ=int((~same & wide).sum()), within_E=int((~wide).sum()),
                   best=_worst(np.abs(best - ref_best)[same], tol))
        if k == 1:
            fig["second"] = 0.0 if np.isneginf(second).all() else np.inf
        else:
            fig["second"] = _worst(np.abs(second - ref_second)[same], tol)
    return fig


def assign_failures(fig):
    bad = []
    if fig["inadmissible"] or fig["differ"]:
        bad.append(f"{fig['inadmissible']} labels not admissible, {fig['differ']} differ where the margin is wide")
    if not fig["best"] <= 1.0:
        bad.append(f"best off by {fig['best']:.3g} of its tolerance")
    if not fig["second"] <= 1.0:
        bad.append(f"second off by {fig['second']:.3g} of its tolerance")
    return bad


def assign_standin(x, inv, n, d, c32, k, prior=None, beta=0.0, plant=None):
    """kmeans_assign_kernel in float32 NumPy: a lane skips the float4s that start at or beyond d, centre columns >= d are
    zeroed, KP centres are kept.  plant: "half" (the second 256 columns of every 512-column chunk are dropped), "unmasked"
    (centre columns >= d are let through), "kp" (KP one size too small: the centres j >= KP / 2 are lost)"""
    ld = x.shape[1]
    col = np.arange(ld)
    use = col // 4 * 4 < d
    if plant == "half":
        use &= col % 512 < 256
    c = c32[:k].copy()
    if plant != "unmasked":
        c[:, d:] = 0.0
    kk = min(k, kp_of(k) // 2 if plant == "kp" else kp_of(k))
    with np.errstate(invalid="ignore"):
        s = (x[:n][:, use] @ c[:kk][:, use].T).astype(np.float32) * inv[:n, None]
        score = s.copy()
        if prior is not None:
            score = s + np.where(prior[:n, None] == np.arange(kk)[None, :], np.float32(beta), np.float32(0))
        label = np.argmax(score, axis=1).astype(np.int32)
        best = s[np.arange(n), label]
        rest = s.copy()
        rest[np.arange(n), label] = -np.inf
        second = rest.max(axis=1) if kk > 1 else np.full(n, -np.inf, dtype=np.float32)
    return label, best, second


# ------------------------------------------------------------------ 3. update
UPDATE_D = (255, 256, 257, 513)
UPDATE_N = (63, 64, 65, 2048, 2049, 2113)
UPDATE_K = (1, 5, 16)
KM_MAX_ROW_BLOCKS, KM_MIN_BLOCK_ROWS = 32, 64
_update = {}


def row_blocks(n: int):
    """(row blocks, rows per block) of strotss_kmeans_update"""
    nb = min(KM_MAX_ROW_BLOCKS, -(-n // KM_MIN_BLOCK_ROWS))
    return nb, -(-n // nb)


def update_data(d, n, k):
    """(x, inv, label, start (k, ld) float32, want (k, d) float64, want_count): planted rows under their planted labels with
    cluster k - 1 emptied (k >= 2) and labels k and -1 on two rows of the first and of the last row block; the centres start
    at random values with 7 in their padding"""
    if (d, n, k) not in _update:
        x, planted = KR.planted_rows(n, d, k, 1.0, 4000 + d + n + k)
        inv = KR.inv_norm(x, n)
        label = planted.copy()
        if k >= 2:
            label[label == k - 1] = 0
        label[[5, n - 3]], label[[6, n - 2]] = k, -1
        start = np.full((k, x.shape[1]), 7.0, dtype=np.float32)
        start[:, :d] = np.random.default_rng(d + n + k).random((k, d))
        want, want_count = KR.update(x, inv, label, n, d, k, start[:, :d])
        _update[(d, n, k)] = (x, inv, label, start, want, want_count)
    return _update[(d, n, k)]


def update_figures(centres, count, want, want_count, start, d):
    """test_update_matches_float64's checks: every updated centre within 2^-24 |want| + 1e-10, its padding +0.0 in its bits, the
    counts exact, an empty cluster's row bit for bit the one it started with"""
    full = want_count > 0
    err = np.abs(centres[full, :d].astype(np.float64) - want[full])
    return dict(centres=_worst(err, U24 * np.abs(want[full]) + 1e-10), count_ok=bool(np.array_equal(count, want_count)),
                padding=int((centres[full, d:].view(np.int32) != 0).sum()),
                empty_moved=int((centres[~full].view(np.int32) != start[~full].view(np.int32)).sum()))


def update_failures(fig):
    bad = []
    if not fig["centres"] <= 1.0:
        bad.append(f"centres off by {fig['centres']:.3g} of their bound")
    if not fig["count_ok"]:
        bad.append("counts differ")
    if fig["padding"]:
        bad.append(f"{fig['padding']} padding values of updated centres are not +0.0")
    if fig["empty_moved"]:
        bad.append(f"{fig['empty_moved']} values of empty clusters' centres changed")
    return bad


def update_standin(x, inv, label, n, d, k, start, plant=None):
    """kmeans_partial_kernel + kmeans_finish_kernel in float64 NumPy: per row block the sums of x inv by label, the blocks
    added in ascending order, c / |c| rounded once.  plant "last_block": the last row block's rows are never added"""
    nb, rows = row_blocks(n)
    total = np.zeros((k, d))
    u = x[:n, :d].astype(np.float64) * inv[:n].astype(np.float64)[:, None]
    for b in range(nb - 1 if plant == "last_block" else nb):
        r0, r1 = b * rows, min(n, (b + 1) * rows)
        for j in range(k):
            total[j] += u[r0:r1][label[r0:r1] == j].sum(axis=0)
    out = start.copy()
    count = np.array([(label[:n] == j).sum() for j in range(k)], dtype=np.int32)
    for j in range(k):
        if count[j]:
            norm = np.sqrt((total[j] * total[j]).sum())
            out[j] = 0.0
            if norm > 0:
                out[j, :d] = (total[j] / norm).astype(np.float32)
    return out, count


# ------------------------------------------------------------------ 4. label warp
# (h, w, gh, gw).  513 cells of 2 or 3 pixels: three workgroups, the last one with a single cell (the shapes of _track_ref run
# 35, 3072 = 12 x 256 and 1 cells: no launch has a full workgroup AND a ragged one); gw == w with gh < h: 1500 cells in six
# workgroups, the probe column is the cell itself
WARP_EDGE_SHAPES = [(40, 50, 19, 27), (15, 300, 5, 300)]


def warp_border_flows(h, w, gh, gw):
    """[(name, flow)]: every probe sent to the first source pixel inside or outside a border -- y_c + dy in {-0.5 -> row 0,
    -0.75 -> row -1, h - 0.75 -> row h - 1, h - 0.5 -> row h}, by cell row, and the same in x by cell column -- and flows of
    +-3e38 and 1e10, which are finite, leave the image and must never reach an integer cast.  All exact in float32."""
    yc, xc = TR.probes(gh, h), TR.probes(gw, w)
    ends_y, ends_x = (-0.5, -0.75, h - 0.75, h - 0.5), (-0.5, -0.75, w - 0.75, w - 0.5)
    rng = np.random.default_rng(h + w + gh + gw)
    base = (rng.integers(-8, 9, size=(h, w, 2)) / 4.0).astype(np.float32)
    fy, fx, huge = base.copy(), base.copy(), base.copy()
    for i in range(gh):
        fy[yc[i], xc, 1] = ends_y[i % 4] - yc[i]
        fy[yc[i], xc, 0] = 0.0
    for j in range(gw):
        fx[yc, xc[j], 0] = ends_x[j % 4] - xc[j]
        fx[yc, xc[j], 1] = 0.0
    values = np.float32([3e38, -3e38, 1e10, -1e10])
    for i in range(gh):
        huge[yc[i], xc, i % 2] = values[(i + np.arange(gw)) % 4]
    return [("border-y", fy), ("border-x", fx), ("huge", huge)]


def warp_edge_cases(h, w, gh, gw, k=TR.WARP_K):
    """_track_ref.warp_cases of the shape, and the border flows on its random grid with and without a certainty"""
    cases = TR.warp_cases(h, w, gh, gw, k)
    grid = cases[0][1]
    ones = np.ones((h, w), np.float32)
    for name, flow in warp_border_flows(h, w, gh, gw):
        cases += [(f"{name}-none", grid, flow, None), (f"{name}-ones", grid, flow, ones)]
    return cases
