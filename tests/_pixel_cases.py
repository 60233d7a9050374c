"""The pixel-side problems the tests run, as seeded cases: sizes, input laws and options for the Laplacian pyramid kernels
(resize, its adjoint, the fused fold and fold adjoint), the first VGG layer and its data-gradient, the max-pool, RMSprop and the
byte output.  A plain module (not a conftest).  tests/test_pixel_cases_cpu.py checks on the CPU that every case has the property
it was built for and that the references of tests/_pixel_ref.py agree with the oracle; tests/test_hip_pixel_path.py runs the
kernels at every case.

Input laws
  image        uniform [0, 1) float32; "blocks": the same with 8 x 8 blocks set to exactly 0.0 and exactly 1.0
  pyramid      level k uniform [-1, 1): the levels are independent, so a fold is not just the image again
  gradients    standard normal float32 (resize adjoint, first-layer data-gradient, pool backward)
  pool input   relu(randn): half exactly zero; planted: every ordered pair of window positions holds a positive tie somewhere,
               and whole windows are zero
  rmsprop      gradient magnitudes log-uniform in [1e-12, 1e3], random sign, one element in sixteen exactly 0
  byte output  see postprocess_input"""
import numpy as np

from _hypercol_cases import ODD

SCHEDULE = [(42, 64), (85, 128), (170, 256), (341, 512), (683, 1024), (1024, 683), (1024, 1024), (64, 64)]
# the first layer's 128-pixel segments: a last segment of 127, 128, 1, 127, 128 and 1 pixels, heights that are no multiple of 4
SEGMENT_EDGES = [(h, w) for h in (5, 17) for w in (127, 128, 129, 255, 256, 257)]
IMAGE_SIZES = SCHEDULE + ODD                      # 683 x 911: 683 * 8 = 5464 trips > 2048 and 911 % 128 != 0
FIRST_LAYER_SIZES = IMAGE_SIZES + SEGMENT_EDGES
SWEEP_MAX = 2050
SWEEP_OTHER = 5
PYRAMID_LEVELS = 5                                # make_laplacian_pyramid: 5 halvings, 6 tensors


def chain(h, w, levels=PYRAMID_LEVELS):
    """the level sizes make_laplacian_pyramid builds"""
    out = [(h, w)]
    for _ in range(levels):
        h, w = max(h // 2, 1), max(w // 2, 1)
        out.append((h, w))
    return out


def sweep_sizes():
    """every length 1 .. SWEEP_MAX on one axis with SWEEP_OTHER on the other, both orientations"""
    return [(n, SWEEP_OTHER) for n in range(1, SWEEP_MAX + 1)] + [(SWEEP_OTHER, n) for n in range(1, SWEEP_MAX + 1)]


# pyramids the one-launch fold must refuse (the caller folds level by level): the first is the issue's example (100 -> 90 shrinks
# too little for the 24-pixel region), the second grows
REFUSED_PYRAMIDS = [[(100, 75), (90, 70), (30, 20)], [(40, 40), (20, 20), (30, 30)]]
# (ih, iw, oh, ow, c): the resize forward beyond the pyramids' 2x steps
RESIZE_RATIOS = [(321, 481, 42, 64, 3), (1500, 2000, 48, 64, 3), (321, 481, 42, 64, 1), (683, 1024, 341, 512, 2),
                 (341, 512, 683, 1024, 2), (85, 128, 170, 256, 8), (170, 256, 85, 128, 8), (5, 7, 341, 512, 3),
                 (2, 3, 100, 75, 1), (97, 131, 100, 75, 8), (1, 1, 4, 3, 3), (7, 5, 1, 1, 3)]
# (ih, iw, oh, ow, c) of the adjoint: gin (ih, iw) = resize^T gout (oh, ow).  Strong downscales leave input pixels without a
# contributing output; strong upscales have more than 8 candidate columns (the generic loop)
ADJOINT_RATIOS = [(321, 481, 42, 64, 3), (1500, 2000, 48, 64, 3), (85, 128, 170, 256, 8), (170, 256, 85, 128, 8),
                  (5, 7, 341, 512, 3), (2, 3, 100, 75, 1), (97, 131, 100, 75, 8), (1, 1, 4, 3, 3), (7, 5, 1, 1, 3),
                  (42, 64, 85, 128, 1), (3, 300, 40, 2050, 3)]

POOL_SHAPES = [(683, 1024, 64), (341, 512, 128), (170, 256, 256), (85, 128, 512), (21, 32, 512), (2, 2, 4), (4, 2100, 64)] + \
    [(h, w, 64) for h, w in ODD]

# one call per set.  The ABI takes at most 8 tensors per call (STROTSS_MAX_TENSORS), so the two pyramids are a call each
RMSPROP_SETS = {
    "pyramid_683x1024": [3 * h * w for h, w in chain(683, 1024)],
    "pyramid_683x911": [3 * h * w for h, w in chain(683, 911)],
    "unequal": [1, 2 * 1024 * 1024, 3, 255, 256, 257, 2048 * 256 + 1, 70000],                             # 8 tensors
}
RMSPROP_STEPS = 3
LR, RHO, EPS = 2e-3, 0.99, 1e-8                   # the product's (nn/engine.py); the kernel receives their float32 values

POSTPROCESS_LENGTHS = [683 * 1024 * 3, 683 * 911 * 3, 1024 * 256 * 2 + 77]
POSTPROCESS_LAWS = ("inside", "outside", "integers")
POSTPROCESS_PLANTS = ("first", "last", "tail", "strided")


def seed_of(*key):
    s = 17
    for k in key:
        s = (s * 1000003 + (sum(map(ord, k)) if isinstance(k, str) else int(k))) % (2 ** 31)
    return s


def image(h, w, law="uniform", c=3):
    rng = np.random.default_rng(seed_of("image", h, w, c))
    x = rng.random((h, w, c), dtype=np.float32)
    if law == "blocks":
        for by in range(0, h, 16):
            for bx in range(0, w, 16):
                x[by:by + 8, bx:bx + 8] = np.float32((by // 16 + bx // 16) & 1)
    return x


def pyramid(sizes, seed=0):
    rng = np.random.default_rng(seed_of("pyr", sizes[0][0], sizes[0][1], seed))
    return [(rng.random((h, w, 3), dtype=np.float32) * 2 - 1).astype(np.float32) for h, w in sizes]


def normal(shape, *key):
    return np.random.default_rng(seed_of("normal", *key)).standard_normal(shape, dtype=np.float32)


def pool_input(h, w, c):
    """relu(randn) with planted ties and zero windows.  Window (oy, ox) with (oy * Wo + ox) % 7 == 3 gets, in every channel, the
    value 2.5 at the two positions of pair number ((oy * Wo + ox) // 7) % 6 and smaller positive values elsewhere; windows with
    % 7 == 5 are all zero."""
    rng = np.random.default_rng(seed_of("pool", h, w, c))
    x = np.maximum(rng.standard_normal((h, w, c), dtype=np.float32), 0)
    ho, wo = h // 2, w // 2
    win = np.arange(ho * wo).reshape(ho, wo)
    pairs = [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    v = x[:2 * ho, :2 * wo].reshape(ho, 2, wo, 2, c)
    tie = win % 7 == 3
    for k, (a, b) in enumerate(pairs):
        sel = tie & ((win // 7) % 6 == k)
        for q in range(4):
            v[:, q >> 1, :, q & 1][sel] = np.float32(2.5) if q in (a, b) else np.float32(0.25 * (q + 1))
    zero = win % 7 == 5
    for q in range(4):
        v[:, q >> 1, :, q & 1][zero] = 0
    return x


def pool_base(h, w, c):
    """what gin holds before an accumulating backward: +-[0.5, 1), never zero.  x + (+0.0) == x bit for bit for every x but
    -0.0 (which becomes +0.0), so a base without -0.0 is kept bit for bit wherever the pool routes nothing."""
    rng = np.random.default_rng(seed_of("poolbase", h, w, c))
    return ((rng.random((h, w, c), dtype=np.float32) * 0.5 + 0.5) * rng.choice(np.float32([-1, 1]), (h, w, c))).astype(np.float32)


def rmsprop_gradient(n, step, k):
    """magnitudes log-uniform in [1e-12, 1e3] (the square of the smallest, 1e-24, is a normal float32: gradients whose square
    underflows are left out on purpose, there the relative bound on rms does not hold), one in sixteen exactly 0"""
    rng = np.random.default_rng(seed_of("rms", n, step, k))
    g = 10.0 ** rng.uniform(-12, 3, n) * rng.choice([-1.0, 1.0], n)
    g[rng.random(n) < 1.0 / 16] = 0.0
    return g.astype(np.float32)


def postprocess_input(n, law, plant):
    """two float32 vectors of length n.  inside: everything in (0.2, 0.8), the extremes 0.125 and 0.875 planted; outside: values
    from -0.5 to 1.5, so the clip produces the extremes 0 and 1 in many places, and -3 and 7 planted; integers: k / 255 for k in
    1 .. 254 with 0 and 1 planted, so the range is 1 and v * 255 lands on or next to an integer, where the truncating cast is
    sensitive to the last bit.  The first vector has the minimum where `plant` says and the maximum elsewhere, the second the
    maximum there: first element, last element, the tail beyond the last full 256 (the last block where the length is a multiple of 256), an index beyond 1024 x 256 that only the
    grid-stride loop reaches."""
    rng = np.random.default_rng(seed_of("post", n, law, plant))
    if law == "inside":
        x, lo, hi = rng.uniform(0.2, 0.8, n), 0.125, 0.875
    elif law == "outside":
        x, lo, hi = rng.uniform(-0.5, 1.5, n), -3.0, 7.0
    else:
        x, lo, hi = rng.integers(1, 255, n) / 255.0, 0.0, 1.0
    x = x.astype(np.float32)
    assert n > 1024 * 256 + 4321
    where = {"first": 0, "last": n - 1, "tail": n - 1 - ((n % 256) // 2 if n % 256 else 100), "strided": 1024 * 256 + 4321}[plant]
    other = {"first": n // 2, "last": n // 3, "tail": 5, "strided": n - 2}[plant]
    out = []
    for a, b in ((lo, hi), (hi, lo)):
        y = x.copy()
        y[where], y[other] = a, b
        out.append(y)
    return out
