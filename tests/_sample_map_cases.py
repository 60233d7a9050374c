"""Seeded cases of the weighted index draw (--sample_map), shared by test_sample_map_cpu.py (the
host twin's own properties) and test_hip_sample_map.py (strotss_index_draw_weighted against the host twin, element for
element).  A case is one call: per region a level map (uint16 (h, w), or None: that region draws uniformly) and a mask
(bool (h, w), or None), region r drawing number t0 + r of the stream with key `seed`, the counters advancing by `stride`.
Every shape is small: the largest grid, 181 x 181, is the 32761 candidates just under the kernel's 32768."""
import functools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SAMPLE_SIZE = 1024
THRESHOLD_A = (0, 1, 1023, 1024, 1025, 4096)


def _mask(h, w, share, seed):
    """a blocky boolean mask with about `share` of the pixels kept"""
    rng = np.random.default_rng(seed)
    return rng.random((h, w)) < share


def _flat(h, w, value):
    return np.full((h, w), value, dtype=np.uint16)


def _random_levels(h, w, seed):
    return np.random.default_rng(seed).integers(0, 65536, size=(h, w), dtype=np.uint16)


def two_level_map(a: int, h: int = 64, w: int = 64, seed: int = 5) -> np.ndarray:
    """exactly `a` cells of 65535 (always accepted), 0 (never accepted) elsewhere: the accepted count is `a`, whatever the draw"""
    q = np.zeros(h * w, dtype=np.uint16)
    q[np.random.default_rng(seed).permutation(h * w)[:a]] = 65535
    return q.reshape(h, w)


def halves_map(h: int = 64, w: int = 64) -> np.ndarray:
    """left half 65535, right half 16384: acceptance exactly 1 and exactly 1/4"""
    q = np.full((h, w), 16384, dtype=np.uint16)
    q[:, : w // 2] = 65535
    return q


def _case(name, h, w, regions, seed=0, t0=0, n=SAMPLE_SIZE, stride=None):
    return dict(name=name, h=h, w=w, n=n, seed=seed, t0=t0, regions=regions, stride=len(regions) if stride is None else stride)


def _build():
    cases = []
    # ---- identities: all 65535 and all 0 give the unweighted draw
    for value in (65535, 0):
        cases.append(_case(f"flat{value}_64x64", 64, 64, [(_flat(64, 64, value), None)], seed=1, t0=3))
        cases.append(_case(f"flat{value}_181x181", 181, 181, [(_flat(181, 181, value), None)], seed=2, t0=0))
        cases.append(_case(f"flat{value}_300x200", 300, 200, [(_flat(300, 200, value), None)], seed=3, t0=17))
        cases.append(_case(f"flat{value}_37x75_masked", 37, 75, [(_flat(37, 75, value), _mask(37, 75, 0.6, 21))], seed=4, t0=9))
    # ---- the accepted count on the threshold between the two passes
    for a in THRESHOLD_A:
        cases.append(_case(f"two_level_A{a}", 64, 64, [(two_level_map(a), None)], seed=10 + a, t0=a))
    # ---- random levels
    cases.append(_case("random_64x64", 64, 64, [(_random_levels(64, 64, 31), None)], seed=31, t0=1))
    cases.append(_case("random_45x65", 45, 65, [(_random_levels(45, 65, 32), None)], seed=32, t0=2))
    cases.append(_case("random_181x181", 181, 181, [(_random_levels(181, 181, 33), None)], seed=2 ** 63 + 33, t0=2 ** 32 - 1))
    cases.append(_case("random_20x30", 20, 30, [(_random_levels(20, 30, 34), None)], seed=34, t0=4))
    cases.append(_case("random_64x64_mask_few", 64, 64, [(_random_levels(64, 64, 35), _mask(64, 64, 0.2, 35))], seed=35, t0=5))
    cases.append(_case("random_64x64_mask_many", 64, 64, [(_random_levels(64, 64, 36), _mask(64, 64, 0.6, 36))], seed=36, t0=6))
    cases.append(_case("random_300x200_n100", 300, 200, [(_random_levels(300, 200, 37), None)], seed=37, t0=7, n=100))
    # ---- three regions in one call: levels on 0 and 2, none on 1, each with its own mask
    cases.append(_case("three_regions", 96, 80, [(_random_levels(96, 80, 41), _mask(96, 80, 0.5, 41)),
                                                 (None, _mask(96, 80, 0.4, 42)),
                                                 (halves_map(96, 80), _mask(96, 80, 0.1, 43))], seed=41, t0=100, stride=3))
    return cases


CASES = _build()
CASE_NAMES = [c["name"] for c in CASES]
BY_NAME = {c["name"]: c for c in CASES}
assert int(_mask(64, 64, 0.2, 35).sum()) < SAMPLE_SIZE < int(_mask(64, 64, 0.6, 36).sum())


def host_region(case, r: int, weighted: bool = True) -> np.ndarray:
    """region r's coordinates from the host twin (weighted=False: the unweighted draw of the same draw number)"""
    from nn import rand as RAND, strotss_utils as SU
    levels, mask = case["regions"][r]
    stream = RAND.PhiloxStream(case["seed"], case["t0"] + r)
    if weighted and levels is not None:
        out = SU.make_indices_weighted_np(case["h"], case["w"], case["n"], stream, levels, mask)
    else:
        out = SU.make_indices_np(case["h"], case["w"], True, case["n"], stream, mask)
    assert stream.t == case["t0"] + r + 1
    return out


@functools.lru_cache(maxsize=None)
def host_reference(name: str):
    """the host twin's coordinates of every region of a case, computed once and shared (read-only)"""
    outs = tuple(host_region(BY_NAME[name], r) for r in range(len(BY_NAME[name]["regions"])))
    for o in outs:
        o.setflags(write=False)
    return outs


def inclusion_ratio(draws) -> float:
    """the proportionality statistic on halves_map(64, 64): per-candidate inclusion frequency of the left half (level 65535)
    over the right half (level 16384); both halves have the same number of candidates.  draws: (n, 2) coordinate arrays."""
    left = sum(int((d[:, 1] < 32).sum()) for d in draws)
    right = sum(int((d[:, 1] >= 32).sum()) for d in draws)
    return left / right
