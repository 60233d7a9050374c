"""The hypercolumn sampling problems the tests run, as seeded cases: image size, index set, feature-gradient law and call options.
A plain module (not a conftest).  tests/test_hypercol_cases_cpu.py checks on the CPU that every case has the property it was
built for and that the reference of tests/_hypercol_ref.py agrees with the oracle on it; tests/test_hip_hypercol.py runs the
gathers and the three tap adjoints at every case on the product's ten maps (3, 64, 64, 128, 128, 256, 256, 256, 512, 512
channels at pool levels 0, 0, 0, 1, 1, 2, 2, 2, 3, 4).

A case does not hold its maps (265 M floats at 1024 x 1024): `fill_maps` / `fill_base` make them on the device from the case's
seed, and the reference reads back the pixels the taps touch.  Laws:
  maps      map 0 (never masked) standard normal, the trunk's maps relu(randn): about half of a masked map is exactly zero
  gradient  "signed": +-[0.5, 1.5) with one element in sixteen exactly zero (the adjoint skips zero products);
            "int": integers in [-8, 8] (with integer positions on an all-2.0 size every product and partial sum is exact in f32)
  base      what the gradient maps hold before the adjoint adds to them: +-[0.5, 1), the size of the gradients themselves, or
            integers +-[1, 8] with "int".  The bound (m + 2)u B + u|base + ref| charges ONE rounding at the size of the base.
            That is what the dense blocks and the sorted form do: they sum first and add once.  The atomic form adds each of its
            m products onto the destination, so m - 1 more roundings happen at the size of base + partial sum, which the bound
            does not count; they fit in its spare 2u B when (m - 1)|base| <= 2B.  So for the atomic form only, and only at
            elements with m >= 2 entries, the base's magnitude is capped at B / m (tests/_hypercol_worker.py: base_for), a law
            made from the reference's own m and B: then products (u B), m - 1 adds (< u(m - 1)(B / m + B)) and the last add
            stay below (m + 1)u B + u|base + ref|.  The capped base is still 1 / (m (m + 2) u) bounds tall, so an adjoint
            that overwrote instead of adding misses by far; elements with one entry keep the full base."""
import collections

import numpy as np

from oracle import strotss_oracle as O

ALL2 = [(1024, 1024), (683, 1024), (1024, 683), (341, 512), (170, 256), (85, 128), (42, 64), (64, 64)]   # divisors all 2.0
ODD = [(683, 911), (767, 1023), (341, 455), (100, 75), (75, 100), (97, 131)]                            # both sides odd somewhere
WINDOW_ROWS = (256, 512)                   # the image rows a strip of 683 x 1024 holds
SAMPLE_RANGE = (37, 700)

Case = collections.namedtuple("Case", "label h w kind n grad seed sample_range window")


def _case(hw, kind, n=1024, grad="signed", sample_range=None, window=None, seed=[100]):
    seed[0] += 1
    label = f"{hw[0]}x{hw[1]}_{kind}" + (f"_n{n}" if n != 1024 else "") + ("_exact" if grad == "int" else "") + \
        ("_range" if sample_range else "") + ("_window" if window else "")
    return Case(label, hw[0], hw[1], kind, n, grad, seed[0], sample_range, window)


CASES = (
    # a. the product's draw (integer positions on the strided grid), every size
    [_case(hw, "draw") for hw in ALL2 + ODD]
    # b. the draw with the four corners and the last row and column forced in: clipped and duplicated taps
    + [_case(hw, "edges") for hw in [(683, 1024), (1024, 683), (341, 512), (85, 128), (42, 64)] + ODD]
    # c. any float position: the general bilinear case on the level-0 maps, all 4096 plan entries valid
    + [_case(hw, "float") for hw in [(1024, 1024), (683, 1024), (64, 64), (683, 911), (767, 1023), (100, 75), (75, 100), (97, 131)]]
    # d. every sample on one pixel / on two neighbouring pixels: one plan segment of 4096 entries, a full dense list
    + [_case(hw, kind) for hw in [(1024, 1024), (683, 1024), (85, 128), (42, 64), (64, 64), (683, 911), (97, 131)]
       for kind in ("one_pixel", "two_pixels")]
    # e. fewer samples than 1024 (mask regions)
    + [_case(hw, "draw", n=n) for hw in [(683, 1024), (64, 64), (100, 75)] for n in (1, 37, 1000)]
    # f. exact sums
    + [_case(hw, "draw", grad="int") for hw in [(1024, 1024), (683, 1024), (170, 256), (64, 64)]]
    # a device-side sample_range
    + [_case((683, 1024), "draw", sample_range=SAMPLE_RANGE), _case((683, 911), "float", sample_range=SAMPLE_RANGE),
       _case((85, 128), "edges", sample_range=SAMPLE_RANGE)]
    # windowed maps (a strip of the image), with and without a sample_range
    + [_case((683, 1024), "draw", window=WINDOW_ROWS), _case((683, 1024), "float", window=WINDOW_ROWS),
       _case((683, 1024), "edges", window=WINDOW_ROWS, sample_range=SAMPLE_RANGE)]
)
LABELS = [c.label for c in CASES]
assert len(set(LABELS)) == len(LABELS)
BY_LABEL = {c.label: c for c in CASES}
EXACT = [c.label for c in CASES if c.grad == "int"]
WINDOWED = [c.label for c in CASES if c.window]
# the cases the atomic adjoint also runs with its dense blocks switched off and widened to 4096 pixels (one child process per
# setting): every case whose maps the default or the widened limit concerns, short of repeating all index sets at every size
DENSE_SWITCH = [c.label for c in CASES if not c.window and (c.h * c.w <= 170 * 256 or (c.h, c.w, c.kind) in
                                                             {(1024, 1024, "draw"), (683, 1024, "one_pixel"), (683, 1024, "edges"),
                                                              (683, 911, "float")})]


def indices(case):
    """(n, 2) float32 (row, col)"""
    h, w, n = case.h, case.w, case.n
    rng = np.random.default_rng(case.seed)
    if case.kind in ("draw", "edges"):
        idx = O.make_indices(h, w, True, n, rng)
        assert idx.shape == (n, 2) and np.array_equal(idx, np.floor(idx))
        if case.kind == "edges":
            idx[:4] = [(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)]
            idx[4:36, 0], idx[4:36, 1] = h - 1, rng.integers(0, w, 32)
            idx[36:68, 0], idx[36:68, 1] = rng.integers(0, h, 32), w - 1
            idx = idx[rng.permutation(n)]
        return idx
    if case.kind == "float":
        return (rng.random((n, 2)) * [h - 1, w - 1]).astype(np.float32)
    if case.kind == "one_pixel":
        # the last pixel: on every pooled map all four taps clip onto ONE pixel with four non-zero weights
        return np.tile(np.float32([[h - 1, w - 1]]), (n, 1))
    if case.kind == "two_pixels":
        r, c = (h // 2) | 1, (w // 2) | 1
        idx = np.tile(np.float32([[r, c]]), (n, 1))
        idx[1::2, 1] += 1
        return idx
    raise ValueError(case.kind)


def gradient(case, d):
    """(n, d) float32 feature gradients"""
    rng = np.random.default_rng(case.seed + 7000)
    if case.grad == "int":
        return rng.integers(-8, 9, (case.n, d)).astype(np.float32)
    g = rng.uniform(0.5, 1.5, (case.n, d)) * rng.choice([-1.0, 1.0], (case.n, d))
    g[rng.random((case.n, d)) < 1.0 / 16] = 0.0
    return g.astype(np.float32)


def windows(case, shapes, levels):
    """per map (row0, rows) of the case's strip, or None"""
    if not case.window:
        return None
    r0, r1 = case.window
    return [(r0 >> l, (r1 >> l) - (r0 >> l)) for l in levels]


def fill_maps(case, shapes, chans, device, dtype=None):
    """the maps, made on `device` from the case's seed: list of (1, h, w, c)"""
    import torch
    gen = torch.Generator(device=device).manual_seed(case.seed)
    out = []
    for k, ((h, w), c) in enumerate(zip(shapes, chans)):
        m = torch.randn((1, h, w, c), generator=gen, device=device, dtype=dtype or torch.float32)
        out.append(m if k == 0 else torch.relu(m))
    return out


def fill_base(case, shapes, chans, device):
    """what the gradient maps hold before the adjoint: never zero"""
    import torch
    gen = torch.Generator(device=device).manual_seed(case.seed + 9000)
    out = []
    for (h, w), c in zip(shapes, chans):
        sign = torch.randint(0, 2, (1, h, w, c), generator=gen, device=device).float() * 2 - 1
        if case.grad == "int":
            mag = torch.randint(1, 9, (1, h, w, c), generator=gen, device=device).float()
        else:
            mag = torch.rand((1, h, w, c), generator=gen, device=device) * 0.5 + 0.5
        out.append(sign * mag)
    return out
