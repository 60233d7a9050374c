"""The convolution routes the product runs, as cases: (route, direction, h, w, cin, cout) of one generic 3x3 layer
cin -> cout at h x w, where `direction` is "fwd" or "dgrad" and `route` is what `nn.model.conv_route` answers for it.
A plain module (not a conftest): tests/test_route_cases_cpu.py checks on the CPU that every case still routes as labelled
(a policy change then names the case to re-pick), tests/test_hip_conv_routes.py runs each case against float64.

DEFAULT_CASES hold under the default policy (no STROTSS_* switch set).  SWITCH_CASES hold under the switches of their
group, which the library reads once per process: they run in a child process with exactly that environment."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ROUTES = ("direct", "direct_splitk", "F2_gemm_f32", "F4_fused_f32", "F4_gemm_f32", "F4_x3_gemm_128", "F4_x3_gemm_64")

# every generic layer of content_im.jpg at its 683 x 1024 scale, both directions
_SCALE_1024 = [
    ("F4_fused_f32", "F4_fused_f32", 683, 1024, 64, 64),            # block1_conv2
    ("F4_fused_f32", "F4_fused_f32", 341, 512, 64, 128),            # block2_conv1
    ("F4_fused_f32", "F4_fused_f32", 341, 512, 128, 128),           # block2_conv2
    ("F4_x3_gemm_128", "F4_fused_f32", 170, 256, 128, 256),         # block3_conv1
    ("F4_x3_gemm_128", "F4_x3_gemm_128", 170, 256, 256, 256),       # block3_conv2 / conv3
    ("F4_x3_gemm_64", "F4_fused_f32", 85, 128, 256, 512),           # block4_conv1
    ("F4_x3_gemm_64", "F4_x3_gemm_64", 85, 128, 512, 512),          # block4_conv2 / conv3
    ("F4_gemm_f32", "F4_gemm_f32", 42, 64, 512, 512),               # block5_conv1 .. conv3
]

DEFAULT_CASES = [c for f, d, h, w, ci, co in _SCALE_1024 for c in ((f, "fwd", h, w, ci, co), (d, "dgrad", h, w, ci, co))] + [
    # split-K direct: ragged h % 4 / w % 4, the 170 x 256 scale's block5, a short-K layer
    ("direct_splitk", "fwd", 33, 20, 64, 64),
    ("direct_splitk", "dgrad", 33, 20, 64, 64),
    ("direct_splitk", "fwd", 13, 17, 256, 256),
    ("direct_splitk", "dgrad", 13, 17, 256, 256),
    ("direct_splitk", "fwd", 10, 16, 512, 512),
    ("direct_splitk", "dgrad", 10, 16, 512, 512),
    # one-pass direct: the data-gradient of a layer with few output channels (the library sees 64 -> 512 channels)
    ("direct", "dgrad", 21, 64, 512, 64),
    ("direct", "dgrad", 31, 41, 512, 128),
    # F(2x2,3x3): 341 x 512's block5 and 170 x 256's block4, ragged
    ("F2_gemm_f32", "fwd", 21, 33, 512, 512),
    ("F2_gemm_f32", "dgrad", 21, 33, 512, 512),
    ("F2_gemm_f32", "fwd", 23, 29, 256, 512),
    ("F2_gemm_f32", "dgrad", 23, 29, 256, 512),
    # F(4x4,3x3) on the f32 GEMMs, ragged
    ("F4_gemm_f32", "fwd", 43, 61, 256, 512),
    ("F4_gemm_f32", "dgrad", 43, 61, 256, 512),
    ("F4_gemm_f32", "dgrad", 85, 128, 128, 256),
    # fused: 374 work items (> 256: several per workgroup, cross-item prefetch; 374 % 8 != 0: uneven per-XCD ranges)
    ("F4_fused_f32", "fwd", 170, 520, 64, 64),
    ("F4_fused_f32", "dgrad", 170, 520, 64, 64),
    ("F4_fused_f32", "fwd", 171, 259, 64, 128),
    ("F4_fused_f32", "dgrad", 171, 259, 128, 128),
    # bf16x3 GEMMs on 128 x 128 and on 64 x 64 tiles, ragged
    ("F4_x3_gemm_128", "fwd", 170, 255, 256, 256),
    ("F4_x3_gemm_128", "dgrad", 170, 255, 256, 256),
    ("F4_x3_gemm_64", "fwd", 61, 67, 512, 512),
    ("F4_x3_gemm_64", "dgrad", 61, 67, 512, 512),
    # the three F(4x4,3x3) GEMM routes at an ODD tile count T = ceil(h/4) ceil(w/4) (2795, 289, 187): T % 8 != 0 for the x3
    # input transform's 8-tile groups, T % 128 != 0 and T % 64 != 0 for the GEMMs' row tiles (61 x 65 has T = 272);
    # none has fewer multiply-adds than its route's ragged case above, which stays the smallest of its (route, direction)
    ("F4_x3_gemm_128", "fwd", 169, 257, 256, 256),
    ("F4_x3_gemm_128", "dgrad", 169, 257, 256, 256),
    ("F4_x3_gemm_64", "fwd", 65, 65, 512, 512),
    ("F4_x3_gemm_64", "dgrad", 65, 65, 512, 512),
    ("F4_gemm_f32", "fwd", 41, 65, 256, 512),
    ("F4_gemm_f32", "dgrad", 41, 65, 256, 512),
]

SWITCH_CASES = {
    # the f32 GEMM fallback: st_gemm_nt_batched's 128 x 128 tiles with and without the tail split, its 128 x 64 branch
    "x3_off": ({"STROTSS_X3": "0"}, [
        ("F4_gemm_f32", "fwd", 64, 128, 512, 512),
        ("F4_gemm_f32", "dgrad", 64, 128, 512, 512),
        ("F4_gemm_f32", "fwd", 96, 128, 512, 512),
        ("F4_gemm_f32", "dgrad", 96, 128, 512, 512),
        ("F4_gemm_f32", "fwd", 64, 64, 512, 512),
        ("F4_gemm_f32", "dgrad", 64, 64, 512, 512),
    ]),
    # the switches of test_step_parity_with_the_fused_winograd_kernel_forced's second child: block1_conv2 at 64 px on the
    # bf16x3 GEMMs with 64 channels on both sides (by default the fused kernel takes every 64-channel layer)
    "x3_64_channels": ({"STROTSS_DIRECT_MAX_TILES": "0", "STROTSS_WINO_FUSED": "0", "STROTSS_X3_MIN_TILES": "100"}, [
        ("F4_x3_gemm_64", "fwd", 64, 64, 64, 64),
        ("F4_x3_gemm_64", "dgrad", 64, 64, 64, 64),
        ("F4_x3_gemm_64", "fwd", 42, 64, 64, 64),
        ("F4_x3_gemm_64", "dgrad", 42, 64, 64, 64),
    ]),
    # no Winograd at all: the one-pass direct kernel forward (no default route sends a forward there)
    "winograd_off": ({"STROTSS_WINOGRAD": "0"}, [
        ("direct", "fwd", 45, 67, 512, 512),
        ("direct", "dgrad", 45, 67, 512, 512),
        ("direct", "fwd", 75, 90, 64, 128),
    ]),
}


def case_id(case) -> str:
    route, direction, h, w, cin, cout = case
    return f"{route}-{direction}-{h}x{w}x{cin}to{cout}"


def _model():
    for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    from nn import model
    return model


def route_of(case) -> str:
    """What the policy of THIS process's environment answers for the case's layer and direction."""
    _, direction, h, w, cin, cout = case
    return _model().conv_route(h, w, cin, cout, dgrad=direction == "dgrad")


def misrouted(cases):
    """The cases whose label no longer matches the policy, as (case id, route now taken)."""
    return [(case_id(c), r) for c in cases for r in [route_of(c)] if r != c[0]]


def routes_at(h: int, w: int, vgg_type: str = "16"):
    """The set of routes the generic layers of a VGG trunk take at image size h x w, forward and data-gradient."""
    M = _model()
    out = set()
    for it in M.vgg_config(vgg_type):
        if it == "pool":
            h, w = h // 2, w // 2
            continue
        _, cin, cout = it
        if cin != 3:
            out.update((M.conv_route(h, w, cin, cout), M.conv_route(h, w, cin, cout, dgrad=True)))
    return out
