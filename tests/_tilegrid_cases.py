"""The tile-grid sweeps of the loss GEMMs (csrc/gemm.hip, csrc/mfma_x3.h), as case lists and seeded row builders.
A plain module (not a conftest): tests/test_tilegrid_cases_cpu.py checks on the CPU that the lists enumerate what they claim
and that the float64 references can tell a misplaced tile; tests/test_hip_tilegrid.py runs them on the GPU.

Which map from workgroup id to output tile a launch gets depends only on its tile grid (g, gs) = (ceil(n / 64), ceil(ns / 64))
(on ceil(ld / 128) for the covariance), so every sweep below is over grids, with a width as small as the main loops allow.

1. COSINE: strotss_cosine_distance_x3 / strotss_cosine_distance at every (g, gs), g = 1..16 (prediction rows, the A operand),
   gs = 1..33 (style rows), d = 35 (ld = 64: two K-steps of 32), in three edge variants (VARIANTS); SYMM: x == y at every g.
2. GROUP / BLEND: the grouped forward launches against the separate entries at d = 67.
3. MOMENT: the upper-triangular 128 x 128 covariance grid at ceil(ld / 128) = 1..18.

Rows are _loss_cases.hyper_rows: distinct rows at levels of their own, so the cosine distances spread over most of [0, 1] and a
tile written to the wrong place is wrong by O(0.1).  sweep_rows() redraws until no two rows of one matrix are closer than
SEPARATION in cosine distance (the CPU half asserts it)."""
import functools

import numpy as np

import _loss_ref as LR
from _loss_cases import hyper_rows

TILE = 64
# ------------------------------------------------------------------ 1. the cosine products
D_SWEEP = 35                      # ld = 64: the narrowest width with more than one K-step
G_MAX, GS_MAX = 16, 33            # n <= 1024 prediction rows, ns <= 2112 style rows
N_PRED, N_STYLE = TILE * G_MAX, TILE * GS_MAX
SEPARATION = 100.0 * LR.EPS_COST  # no two rows of one matrix closer than this: swapped tiles show
SENTINEL_BITS = 0x7FC0BEEF        # a quiet NaN with a payload: what C holds before a launch
C_EXTRA_ROWS, C_EXTRA_COLS = 8, 32   # C is (nx + 8, pad32(ny) + 32)
VARIANTS = ("exact", "single", "mixed")


def pad32(v):
    return (v + 31) // 32 * 32


def tiles(n):
    return -(-n // TILE)


@functools.lru_cache(maxsize=None)
def _mixed_offsets():
    """rows in the last tile of the mixed variant: one offset in 2..63 per g and one per gs (seeded)"""
    rng = np.random.default_rng(4100)
    return tuple(int(v) for v in rng.integers(2, TILE, G_MAX)), tuple(int(v) for v in rng.integers(2, TILE, GS_MAX))


def rows_of(variant, g, style=False):
    """row count whose tile grid has g tiles: the last tile full ('exact'), one row ('single'), a seeded count ('mixed')"""
    if variant == "exact":
        return TILE * g
    if variant == "single":
        return TILE * (g - 1) + 1
    assert variant == "mixed"
    return TILE * (g - 1) + _mixed_offsets()[1 if style else 0][g - 1]


def cosine_cases(variant):
    """[(g, gs, n, ns)] for every grid of the sweep"""
    return [(g, gs, rows_of(variant, g), rows_of(variant, gs, True)) for g in range(1, G_MAX + 1) for gs in range(1, GS_MAX + 1)]


def symm_cases():
    """[(variant, g, n)]: x == y launches, every g in every variant"""
    return [(v, g, rows_of(v, g)) for v in VARIANTS for g in range(1, G_MAX + 1)]


def _separated(seed, m, d):
    x = hyper_rows(np.random.default_rng(seed), m, d)
    for attempt in range(50):
        D = LR.cos_dist(x, x)
        bad = np.unique(np.nonzero(np.triu(D < SEPARATION, 1))[1])       # the later row of every close pair
        if not len(bad):
            return x
        r2 = np.random.default_rng([seed, attempt + 1])
        for i in bad:
            x[i] = hyper_rows(r2, 1, d)[0]
    raise AssertionError(f"rows of seed {seed} not separated after 50 redraws")


@functools.lru_cache(maxsize=None)
def sweep_rows():
    """(prediction rows (1024, 35), style rows (2112, 35)); a case takes leading rows"""
    return _separated(4000, N_PRED, D_SWEEP), _separated(4001, N_STYLE, D_SWEEP)


@functools.lru_cache(maxsize=None)
def sweep_refs():
    """float64 (prediction x style cosine distances (1024, 2112), prediction self-distances (1024, 1024)): entry (i, j) depends
    on rows i and j only, so a case's reference is the leading (n, ns) block.  Computed once, never written to."""
    pred, style = sweep_rows()
    cross, self_ = LR.cos_dist(pred, style), LR.cos_dist(pred, pred)
    cross.setflags(write=False); self_.setflags(write=False)
    return cross, self_


# ------------------------------------------------------------------ 2. the grouped launches
D_GROUP = 67
GROUP_N = (1, 37, 63, 64, 65, 449, 1000, 1024)
GROUP_NS = (33, 64, 65, 300, 777, 1024, 1500, 2048)
GROUP_G = (0.75, 0.5, 1.0, 0.25)          # g_content, g_moment, g_remd, g_palette: exact in f32, and so are their products
BLEND_WEIGHTS = (0.5, 0.25, 0.125, 0.125)  # with these weights
# (n, ns per style): k = 1..4; at g = 1 (n = 37) and g = 4 (n = 200) inner problems end off a multiple of 8 workgroups
BLEND_NS = ((65,), (65, 1000), (2048, 64, 777), (65, 1000, 129, 2048))
BLEND_N = (37, 1000, 200)
BLEND_CASES = [(n, ns) for n in BLEND_N for ns in BLEND_NS]
BLEND_TOL = 1e-5          # tests/test_hip_style_blend.py: the one call against the separate entries


def group_cases():
    return [(n, ns) for n in GROUP_N for ns in GROUP_NS]


@functools.lru_cache(maxsize=None)
def group_rows():
    """(prediction rows (1024, 67), content rows (1024, 67), style rows (2048, 67)); a case takes leading rows"""
    return (hyper_rows(np.random.default_rng(4010), 1024, D_GROUP), hyper_rows(np.random.default_rng(4011), 1024, D_GROUP),
            hyper_rows(np.random.default_rng(4012), 2048, D_GROUP))


def pad8(v):
    return (v + 7) // 8 * 8


def host_block(g, gs):
    """(bh, bw, kind) of the full g x gs tile grid as the host chooses it (csrc/gemm.hip: st_cosine_distance_x3,
    st_loss_forward_group_x3, x3_xcd_block), restated for the COVERAGE ACCOUNTING only -- never an oracle.
    kind: 'blocked' | 'rows_mod8' (tiles % 8 != 0) | 'rows_nodiv' (no (bh, bw) divides the grid)."""
    if (g * gs) % 8:
        return 0, 0, "rows_mod8"
    per = g * gs // 8
    best = 0
    for h in range(1, per + 1):
        if per % h or g % h:
            continue
        w = per // h
        if gs % w:
            continue
        if not best or h + w < best + per // best:
            best = h
    return (best, per // best, "blocked") if best else (0, 0, "rows_nodiv")


def symm_workgroups(n):
    """workgroups of the symmetric pair (two upper-triangular grids) of n prediction rows in a grouped launch"""
    g = tiles(n)
    return g * (g + 1)


# ------------------------------------------------------------------ 3. the triangular covariance grid
MOMENT_N = 96
MOMENT_D = (35, 128, 129, 259, 515, 1000, 1281, 1793, 2179)
MOMENT_TOL_LOSS = 2e-5    # tests/test_hip_ops.py::test_losses_fwd_bwd: |l - ref| < 2e-5 max(1, |ref|)


@functools.lru_cache(maxsize=None)
def moment_rows(d):
    """(style rows, prediction rows), both (96, d)"""
    return hyper_rows(np.random.default_rng([4020, d]), MOMENT_N, d), hyper_rows(np.random.default_rng([4021, d]), MOMENT_N, d)


def cov_terms(npad):
    """c of the covariance bound: the f32 additions that one output element goes through in x3_mainloop_k16
    (csrc/mfma_x3.h).  Every K-step of 16 samples issues six MFMAs (the six partial products hh, hm, mh, hl, mm, lh of the
    bf16x3 split) into the same accumulator, each adding 16 products: 6 * npad additions over the npad = round_up(n, 32) rows
    of the transposed panels (the zero rows past n are added too), counted as sequential f32 additions -- the worst case,
    whatever the order inside an MFMA.  + 2 for the rounding of the two centred operands (c = x - mean, one rounding each),
    + 1 for the three dropped partial products (ml + lm + ll <= 2^-26 |x y| < U |x y|), + 2 for alpha = 1.0f / n and the
    multiplication by it."""
    return 6 * npad + 5


def cov_bound(v, npad):
    """(|f32 - f64| bound of every covariance entry, of every mean entry) of strotss_moment_stats on the rows of v:
    cov:  c U (1/n) sum_k |c_ki| |c_kj|  (c = cov_terms)  +  dm_i dm_j (the f32 means are off by dm <= (n + 2) U mean_k |v_ki|;
          the first-order terms vanish because the exactly centred columns sum to zero)  +  U |cov_ij| (the stored result);
    mean: n additions (col_sum_partial_kernel + the fixed-order combine, as sequential) + the division + the result."""
    n = v.shape[0]
    m = v.mean(0)
    cv = np.abs(v - m)
    dm = (n + 2) * LR.U * np.abs(v).mean(0)
    S = (v - m).T @ (v - m) / n
    return cov_terms(npad) * LR.U * (cv.T @ cv) / n + dm[:, None] * dm[None, :] + LR.U * np.abs(S), dm
