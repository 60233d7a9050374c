"""The inventory of capped launches ("Capped launches"), and the cases that take each uncovered one past
its cap.  A capped launch bounds its grid (`min(cap, work / items)`, a `*_MAX_*` constant or a ternary) and lets every workgroup
walk the work beyond the cap; a shape below the cap never runs the second trip of that walk.

This file holds what tests/test_launch_caps_cpu.py (no GPU) and tests/test_hip_launch_caps.py (MI355X) share:
  1. the caps and work counts of csrc restated in Python, each with the source line it restates (the CPU file compares every
     constant with the source by a regular expression);
  2. ROWS, one per capped launch: the ABI entry that reaches it, work(shape), cap, items per workgroup, and either `covered_by`
     (an existing test function, the attribute of its module that holds the shape, the shape) or `case` (a new case);
  3. CASES: per new case the data, the float64 reference and bound of the family's own test files (imported, none new), the
     mask of the walked region (outputs of work items >= cap x items), `judge` (ONE comparison, used on the device's result and
     on the planted one) and `walk_stops` (the reference's result as a walk that stops after its first trip would leave it:
     walked elements keep the pre-fill, a walked sum lacks the walked terms).
Pure host code."""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "strotss-tensorflow_amd", "csrc")
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

INT_MAX = 2 ** 31 - 1
NAN = float("nan")


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------ 1. the constants of csrc, restated
# name -> (file, value): `#define name value` of that file
DEFINES = {
    "COLOR_THREADS": ("color.hip", 256), "COLOR_MAX_BLOCKS": ("color.hip", 2048),                      # color.hip:14, 16
    "CT_THREADS": ("color_transfer.hip", 256), "CT_MAX_BLOCKS": ("color_transfer.hip", 256),           # color_transfer.hip:16, 17
    "SMOOTH_COLS_X": ("smooth.hip", 64), "SMOOTH_COLS_Y": ("smooth.hip", 4),                           # smooth.hip:28, 29
    "SMOOTH_ROW_THREADS": ("smooth.hip", 256), "SMOOTH_MAX_GRID": ("smooth.hip", 1 << 14),             # smooth.hip:30, 34
    "UPS_THREADS": ("smooth.hip", 256), "UPS_PIXELS": ("smooth.hip", 4), "UPS_MAX_GRID": ("smooth.hip", 1 << 12),   # :37, 38, 40
    "DM_COLS_X": ("detail_map.hip", 64), "DM_COLS_Y": ("detail_map.hip", 16), "DM_ROW_THREADS": ("detail_map.hip", 256),
    "DM_MAX_GRID": ("detail_map.hip", 1 << 14), "DM_ROWS_MAX_GRID": ("detail_map.hip", 512),           # detail_map.hip:30, 31
    "DM_SCALE_THREADS": ("detail_map.hip", 256), "DM_SCALE_MAX_GRID": ("detail_map.hip", 1 << 12),     # detail_map.hip:33, 34
    "KM_ASSIGN_THREADS": ("kmeans_assign.h", 512), "KM_ROWS_PER_WAVE": ("kmeans_assign.h", 4),         # kmeans_assign.h:22, 23
    "KM_MAX_GRID": ("kmeans_assign.h", 2048),                                                          # kmeans_assign.h:26
    "KM_MAX_ROW_BLOCKS": ("kmeans.hip", 32), "KM_MIN_BLOCK_ROWS": ("kmeans.hip", 64),                  # kmeans.hip:22, 23
    "RF_THREADS": ("refine.hip", 256), "RF_TILE_W": ("refine.hip", 32), "RF_MAX_GRID": ("refine.hip", 16384),   # refine.hip:25, 26, 32
    "C3F_SEG": ("conv.hip", 128),
}
# name -> (file, a pattern whose group 1 is the bare cap of that launch, value)
BARE = {
    "x3_split_rows": ("gemm.hip", r"x3_split_rows_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 2048),             # gemm.hip:436
    "winograd43_pack": ("winograd_fused.hip", r"winograd43_pack_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 4096),
    "sk_exp": ("losses.hip", r"sk_exp_kernel, dim3\(min\((\d+),", 4096),                                               # losses.hip:1466
    "center_stats": ("losses.hip", r"center_kernel, dim3\(min\((\d+), cdiv\(\(size_t\)s\.rows \* ld / 4, 256\)\)\), dim3\(256\), 0, st, x,", 2048),
    "center_fwd": ("losses.hip", r"center_kernel, dim3\(min\((\d+), cdiv\(\(size_t\)s\.rows \* ld / 4, 256\)\)\), dim3\(256\), 0, st,\n", 2048),
    "splitk_finish": ("conv.hip", r"conv_splitk_finish_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 2048),         # conv.hip:509
    "splitk_finish_pool_x": ("conv.hip", r"conv_splitk_finish_pool_kernel, dim3\(\(unsigned\)min\((\d+),", 64),          # conv.hip:497
    "splitk_finish_unpool_x": ("conv.hip", r"conv_splitk_finish_unpool_kernel, dim3\(\(unsigned\)min\((\d+),", 64),      # conv.hip:504
    "relu_bits": ("conv.hip", r"relu_bits_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 8192),                      # conv.hip:958
    "c3_fwd_mfma": ("conv.hip", r"conv3x3_c3_fwd_mfma_kernel, dim3\(min\((\d+), trips\)\)", 2048),                      # conv.hip:971
    "maxpool_fwd_x": ("conv.hip", r"const dim3 grid\(\(unsigned\)min\((\d+), cdiv\(\(w / 2\) \* \(c / 4\), 256\)\)", 64),   # conv.hip:1061
    "maxpool_fwd_y": ("conv.hip", r"\(unsigned\)min\(h / 2, (\d+)\)\);", 16384),                                        # conv.hip:1061
    "maxpool_bwd": ("conv.hip", r"const dim3 grid\(\(unsigned\)min\(\(size_t\)(\d+), \(total \+ 255\) / 256\)\);", 8192),  # conv.hip:1072
    "maxpool_bwd_code_x": ("conv.hip", r"const dim3 g2\(\(unsigned\)min\((\d+), cdiv\(row_elems, 256\)\)", 64),          # conv.hip:1075
    "maxpool_bwd_code_y": ("conv.hip", r"\(unsigned\)min\(rows, (\d+)\)\);", 16384),                                    # conv.hip:1075
    "wino43_in_x3": ("winograd.hip", r"const size_t tin = \(\(T \+ 7\) / 8\) \* 8 \* \(cin / 4\);\n\s*const dim3 gin\(\(unsigned\)min\(\(size_t\)(\d+),", 16384),
    "wino43_in": ("winograd.hip", r"winograd43_in_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 16384),            # winograd.hip:438
    "wino43_out": ("winograd.hip", r"winograd43_out_kernel, dim3\(\(unsigned\)min\(\(size_t\)(\d+),", 16384),          # winograd.hip:446
    "wino2_in": ("winograd.hip", r"const dim3 gin\(\(unsigned\)min\(\(size_t\)(\d+), \(tin \+ 255\) / 256\)\), gout", 16384),   # winograd.hip:481
    "wino2_out": ("winograd.hip", r", gout\(\(unsigned\)min\(\(size_t\)(\d+), \(tout \+ 255\) / 256\)\);", 16384),      # winograd.hip:481
    "winograd_weights": ("winograd.hip", r"winograd_weights_kernel, dim3\(\(unsigned\)min\(\(long long\)(\d+),", 4096),  # winograd.hip:548
    "resize_y": ("image.hip", r"const dim3 grid\(\(unsigned\)cdiv\(ow, 256\), \(unsigned\)min\(oh, (\d+)\)\);", 32768),  # image.hip:738
    "resize_adjoint_y": ("image.hip", r"const dim3 grid\(\(unsigned\)cdiv\(iw, 256\), \(unsigned\)min\(ih, (\d+)\)\);", 32768),  # :805
    "rmsprop": ("image.hip", r"dim3 grid\(\(unsigned\)\(\(mx \+ 255\) / 256 > (\d+) \?", 2048),                          # image.hip:930
    "postprocess": ("image.hip", r"const int nparts = \(int\)\(\(numel \+ 255\) / 256 > (\d+) \?", 1024),                # image.hip:937
}
WAVE = 64
D = {k: v for k, (_, v) in DEFINES.items()}
B = {k: v for k, (_, _, v) in BARE.items()}
KM_TILE_ROWS = D["KM_ASSIGN_THREADS"] // WAVE * D["KM_ROWS_PER_WAVE"]        # kmeans_assign.h:24
UPS_TILE = D["UPS_THREADS"] * D["UPS_PIXELS"]                                # smooth.hip:39


def define_in_source(name):
    """the value of `#define name ...` in its file: an integer, or (1u << n)"""
    text = open(os.path.join(CSRC, DEFINES[name][0])).read()
    m = re.search(r"^#define %s[ \t]+(\(?[0-9u <]+\)?)[ \t]*(//.*)?$" % name, text, re.M)
    assert m, f"{name}: no #define in {DEFINES[name][0]}"
    expr = m.group(1).replace("u", "").strip()
    assert re.fullmatch(r"\(?\d+( << \d+)?\)?", expr), (name, expr)
    return eval(expr)                                                       # digits, "<<" and parentheses only


def bare_in_source(name):
    file, pattern, _ = BARE[name]
    found = re.findall(pattern, open(os.path.join(CSRC, file)).read())
    assert len(found) == 1, f"{name}: {len(found)} matches of its pattern in {file}"
    return int(found[0])


# the work counts, restated
def smooth_cols_tiles(h, w):                                                 # smooth.hip:44 cols_tiles
    return cdiv(w, D["SMOOTH_COLS_X"]) * cdiv(h, D["SMOOTH_COLS_Y"])


def smooth_rows_tiles(h, w):                                                 # smooth.hip:47 rows_tiles
    return cdiv(w, D["SMOOTH_ROW_THREADS"]) * h


def ups_tiles(H, W):                                                         # smooth.hip:475
    return cdiv(H * W, UPS_TILE)


def dm_cols_tiles(h, w):                                                     # detail_map.hip:37
    return cdiv(w, D["DM_COLS_X"]) * cdiv(h, D["DM_COLS_Y"])


def dm_rows_tiles(h, w):                                                     # detail_map.hip:40
    return cdiv(w, D["DM_ROW_THREADS"]) * h


def dm_scale_groups(h, w):                                                   # detail_map.hip:173
    return cdiv(h * w // 4, D["DM_SCALE_THREADS"])


def color_groups(h, w):                                                      # color.hip:45, color_transfer.hip:91: groups of 4 pixels
    return cdiv(h * w, 4)


def km_tiles(n):                                                             # kmeans_assign.h:157
    return cdiv(n, KM_TILE_ROWS)


def km_row_blocks_wanted(n):                                                 # kmeans.hip:80 row_blocks, before the min
    return cdiv(n, D["KM_MIN_BLOCK_ROWS"])


def rf_tiles(h, w):                                                          # refine.hip:194: tiles of RF_TILE_W x RF_TILE_H
    return cdiv(h, D["RF_THREADS"] // D["RF_TILE_W"]) * cdiv(w, D["RF_TILE_W"])


def relu_bits_words(h, w, c):                                                # conv.hip:957
    return cdiv(h, 4) * cdiv(w, 4) * c


def image_ok(h, w):                                                          # image_size_ok of color.hip, smooth.hip, color_transfer.hip
    return h > 0 and w > 0 and 3 * h * w <= INT_MAX


def wino43_tiles(h, w):
    return cdiv(h, 4) * cdiv(w, 4)


# ------------------------------------------------------------------ 2. the inventory
# kernel, entry, what the cap counts, work(shape) -> count of workgroups wanted (work / items), cap, and the coverage.
# `work` is in the cap's own unit (workgroups, or rows of workgroups for a y cap): past the cap means work > cap.
def _row(kernel, source, entry, cap, work, ok, covered_by=None, case=None, named=True):
    assert (covered_by is not None) + (case is not None) == 1, kernel
    return dict(kernel=kernel, source=source, entry=entry, cap=cap, work=work, ok=ok, covered_by=covered_by, case=case,
                named=named)


SMOOTH_STRIP, SMOOTH_WIDE = (65540, 3), (13112, 257)
UPS_LO, UPS_HI = (65540, 3), (65541, 4)
RESIZE_CASES = [(16385, 2, 32771, 3, 3), (50000, 1, 32769, 1, 1), (8200, 3, 32770, 2, 2)]        # (ih, iw, oh, ow, c): oh > 32768
ADJOINT_CASES = [(32771, 3, 16390, 2, 3), (32769, 1, 40000, 1, 1), (32770, 2, 8200, 3, 2)]       # ih > 32768
POOL_TALL = (32771, 2, 4)                     # h / 2 = 16385 pooled rows and the odd row 32770: 16386 rows of the coded backward
COLOR_STATS_SHAPE = (1, 2 ** 21 + 1)          # the smallest pixel count above 2048 x 1024, and no multiple of 4
RELU_BITS_SHAPE = (1, 5, 2 ** 20 + 1)         # two tiles x 2^20 + 1 channels = 2^21 + 2 words
WEIGHTS_SHAPE = (1025, 1024)                  # n k = 2^20 + 1024 kernels
ASSIGN_PRIOR_SHAPE = (2 ** 16 + 33, 35, 3)    # 2050 tiles of 32 rows
DETAIL_SHAPE = (262160, 17, 2)                # 16385 column tiles, 262160 row tiles, 4353 groups of 1024 pixels

_sm = lambda f: (lambda s: f(*s))
ROWS = [
    # ---- named by the issue as covered: proved by the CPU file
    _row("refine_vote_kernel", "refine.hip:194", "strotss_refine_labels", D["RF_MAX_GRID"], lambda s: rf_tiles(s[0], s[1]),
         lambda s: image_ok(s[0], s[1]),
         covered_by=("test_hip_mask_edges::test_refine_at_its_staging_and_walk_edges", "_mask_edge_cases", "REFINE_CASES", "walks", (131080, 3))),
    _row("refine_cell_mean_kernel", "refine.hip:195", "strotss_refine_labels", D["RF_MAX_GRID"],
         lambda s: cdiv(s[2] * s[3], D["RF_THREADS"] // WAVE), lambda s: image_ok(s[0], s[1]),
         covered_by=("test_hip_mask_edges::test_refine_at_its_staging_and_walk_edges", "_mask_edge_cases", "REFINE_CASES", "walks", (131080, 3, 32771, 3)), named=False),
    _row("upsample_apply_kernel", "smooth.hip:476", "strotss_guided_upsample", D["UPS_MAX_GRID"], _sm(ups_tiles), _sm(image_ok),
         covered_by=("test_hip_upsample::test_more_tiles_than_the_largest_grid", "test_hip_upsample", None, "source", (2099, 2101))),
    _row("color_hist_kernel", "color_transfer.hip:296", "strotss_color_hist", D["CT_MAX_BLOCKS"],
         lambda s: cdiv(color_groups(*s), D["CT_THREADS"]), _sm(image_ok),
         covered_by=("test_hip_color_transfer::test_color_hist_brackets_float64_above_the_grid_cap", "test_hip_color_transfer",
                     "BIG", None, (768, 1024))),
    _row("color_apply_kernel", "color_transfer.hip:335", "strotss_color_transfer_apply", D["CT_MAX_BLOCKS"],
         lambda s: cdiv(color_groups(*s), D["CT_THREADS"]), _sm(image_ok),
         covered_by=("test_hip_color_transfer::test_color_transfer_apply_matches_float64", "test_hip_color_transfer", "IMAGES",
                     "first", (768, 1024)), named=False),
    _row("kmeans_assign_kernel", "kmeans_assign.h:158", "strotss_kmeans_assign", D["KM_MAX_GRID"], lambda s: km_tiles(s[0]),
         lambda s: s[0] > 0, covered_by=("test_hip_cluster::test_assign_matches_float64", "test_hip_cluster", "SHAPES", None,
                                         (2 ** 17 + 37, 35, 3))),
    _row("kmeans_partial_kernel", "kmeans.hip:80", "strotss_kmeans_update", D["KM_MAX_ROW_BLOCKS"],
         lambda s: km_row_blocks_wanted(s), lambda s: s > 0,
         covered_by=("test_hip_mask_edges::test_update_at_its_column_and_row_block_edges", "_mask_edge_cases", "UPDATE_N", None, 2113)),
    # ---- the smoothing passes (new cases: the suite's own walk is one pixel wide and radius 4), then what is covered already,
    # much of it found beyond the issue's list (named=False)
    _row("smooth_cols1_kernel, smooth_cols2_kernel", "smooth.hip:424", "strotss_guided_smooth", D["SMOOTH_MAX_GRID"],
         _sm(smooth_cols_tiles), _sm(image_ok), case="smooth"),
    _row("smooth_rows_kernel<1>, <2>", "smooth.hip:425", "strotss_guided_smooth", D["SMOOTH_MAX_GRID"], _sm(smooth_rows_tiles),
         _sm(image_ok), case="smooth"),
    _row("smooth_cols1_kernel, smooth_cols2_kernel (low resolution)", "smooth.hip:465", "strotss_guided_upsample",
         D["SMOOTH_MAX_GRID"], _sm(smooth_cols_tiles), _sm(image_ok), case="upsample"),
    _row("smooth_rows_kernel<1>, smooth_rows_store_kernel", "smooth.hip:466", "strotss_guided_upsample", D["SMOOTH_MAX_GRID"],
         _sm(smooth_rows_tiles), _sm(image_ok), case="upsample"),
    _row("rmsprop_kernel", "image.hip:930", "strotss_rmsprop_step", B["rmsprop"], lambda n: cdiv(n, 256), lambda n: n > 0,
         covered_by=("test_hip_pixel_path::test_rmsprop_three_steps", "_pixel_cases", "RMSPROP_SETS", "unequal", 2048 * 256 + 1),
         named=False),
    _row("minmax_partial_kernel, postprocess_kernel", "image.hip:937", "strotss_postprocess", B["postprocess"],
         lambda n: cdiv(n, 256), lambda n: n > 0,
         covered_by=("test_hip_pixel_path::test_byte_output", "_pixel_cases", "POSTPROCESS_LENGTHS", None, 1024 * 256 * 2 + 77),
         named=False),
    _row("conv3x3_c3_fwd_mfma_kernel", "conv.hip:971", "strotss_conv3x3_c3_fwd", B["c3_fwd_mfma"],
         lambda s: s[0] * cdiv(s[1], D["C3F_SEG"]), lambda s: s[0] > 0 and s[1] > 0,
         covered_by=("test_hip_pixel_path::test_first_layer_forward", "_pixel_cases", "FIRST_LAYER_SIZES", None, (683, 911))),
    _row("maxpool2_fwd_kernel (x)", "conv.hip:1061", "strotss_maxpool2_fwd", B["maxpool_fwd_x"],
         lambda s: cdiv((s[1] // 2) * (s[2] // 4), 256), lambda s: s[0] >= 2 and s[1] >= 2 and s[2] % 4 == 0,
         covered_by=("test_hip_pixel_path::test_maxpool_values_codes_and_backward", "_pixel_cases", "POOL_SHAPES", None, (4, 2100, 64))),
    _row("maxpool2_bwd_code_kernel (x)", "conv.hip:1075", "strotss_maxpool2_bwd", B["maxpool_bwd_code_x"],
         lambda s: cdiv((s[1] // 2 + s[1] % 2) * (s[2] // 4), 256), lambda s: s[0] >= 2 and s[1] >= 2 and s[2] % 4 == 0,
         covered_by=("test_hip_pixel_path::test_maxpool_values_codes_and_backward", "_pixel_cases", "POOL_SHAPES", None, (4, 2100, 64))),
    _row("maxpool2_bwd_kernel", "conv.hip:1072", "strotss_maxpool2_bwd", B["maxpool_bwd"],
         lambda s: cdiv(s[0] * s[1] * (s[2] // 4), 256), lambda s: s[0] >= 2 and s[1] >= 2 and s[2] % 4 == 0,
         covered_by=("test_hip_pixel_path::test_maxpool_values_codes_and_backward", "_pixel_cases", "POOL_SHAPES", None, (683, 1024, 64))),
    _row("winograd43_pack_kernel", "winograd_fused.hip:513", "strotss_conv3x3_winograd_pack", B["winograd43_pack"],
         lambda s: cdiv(36 * s[4] * s[5], 256), lambda s: s[4] % 32 == 0 and s[5] % 32 == 0,
         covered_by=("test_hip_exact_conv::test_integer_case_is_bit_for_bit", "_exact_cases", "DEFAULT_CASES", None, ("F4_fused_f32", "dgrad", 128, 128, 256, 256))),
    # ---- new cases
    _row("maxpool2_fwd_kernel (y)", "conv.hip:1061", "strotss_maxpool2_fwd", B["maxpool_fwd_y"], lambda s: s[0] // 2,
         lambda s: s[0] >= 2 and s[1] >= 2 and s[2] % 4 == 0, case="maxpool_tall"),
    _row("maxpool2_bwd_code_kernel (y)", "conv.hip:1075", "strotss_maxpool2_bwd", B["maxpool_bwd_code_y"],
         lambda s: s[0] // 2 + s[0] % 2, lambda s: s[0] >= 2 and s[1] >= 2 and s[2] % 4 == 0, case="maxpool_tall"),
    _row("resize_bilinear_kernel (y)", "image.hip:738", "strotss_resize_bilinear", B["resize_y"], lambda s: s[2],
         lambda s: min(s) > 0, case="resize"),
    _row("resize_adjoint_kernel (y)", "image.hip:805", "strotss_resize_bilinear_adjoint", B["resize_adjoint_y"], lambda s: s[0],
         lambda s: min(s) > 0, case="resize_adjoint"),
    _row("color_stats_kernel", "color.hip:169", "strotss_color_stats", D["COLOR_MAX_BLOCKS"],
         lambda s: cdiv(color_groups(*s), D["COLOR_THREADS"]), _sm(image_ok), case="color_stats"),
    _row("relu_bits_kernel", "conv.hip:958", "strotss_relu_bits", B["relu_bits"], lambda s: cdiv(relu_bits_words(*s), 256),
         lambda s: min(s) > 0, case="relu_bits"),
    _row("winograd_weights_kernel", "winograd.hip:548", "strotss_conv3x3_winograd_weights", B["winograd_weights"],
         lambda s: cdiv(s[0] * s[1], 256), lambda s: min(s) > 0, case="winograd_weights", named=False),
    _row("kmeans_assign_kernel (prior)", "kmeans_assign.h:175", "strotss_kmeans_assign_prior", D["KM_MAX_GRID"],
         lambda s: km_tiles(s[0]), lambda s: s[0] > 0, case="assign_prior", named=False),
    _row("detail_cols_kernel", "detail_map.hip:169", "strotss_detail_map", D["DM_MAX_GRID"], lambda s: dm_cols_tiles(s[0], s[1]),
         lambda s: image_ok(s[0], s[1]) and 1 <= s[2] <= 64, case="detail_map"),
    _row("detail_rows_kernel", "detail_map.hip:171", "strotss_detail_map", D["DM_ROWS_MAX_GRID"],
         lambda s: dm_rows_tiles(s[0], s[1]), lambda s: image_ok(s[0], s[1]) and 1 <= s[2] <= 64, case="detail_map"),
    _row("detail_scale_kernel", "detail_map.hip:174", "strotss_detail_map", D["DM_SCALE_MAX_GRID"],
         lambda s: dm_scale_groups(s[0], s[1]), lambda s: image_ok(s[0], s[1]) and 1 <= s[2] <= 64, case="detail_map"),
    # ---- the convolution rows: sampled float64 references in a fresh child process per switch group (CONV_GROUPS below)
    _row("winograd43_in_kernel", "winograd.hip:438", "strotss_conv3x3_winograd_fwd (F4 f32 GEMMs)", B["wino43_in"],
         lambda s: cdiv(wino43_tiles(s[0], s[1]) * (s[2] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0, case="conv_in_f32"),
    _row("winograd43_in_x3_kernel", "winograd.hip:432", "strotss_conv3x3_winograd_fwd (x3 panels)", B["wino43_in_x3"],
         lambda s: cdiv(cdiv(wino43_tiles(s[0], s[1]), 8) * 8 * (s[2] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0,
         case="conv_in_x3"),
    _row("winograd43_in_f32k_kernel", "winograd.hip:428", "strotss_conv3x3_winograd_fwd (x3 f32a)", B["wino43_in_x3"],
         lambda s: cdiv(cdiv(wino43_tiles(s[0], s[1]), 8) * 8 * (s[2] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0,
         case="conv_in_f32k"),
    _row("winograd43_out_kernel", "winograd.hip:446", "strotss_conv3x3_winograd_fwd", B["wino43_out"],
         lambda s: cdiv(wino43_tiles(s[0], s[1]) * (s[3] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0, case="conv_out"),
    _row("winograd_in_kernel", "winograd.hip:482", "strotss_conv3x3_winograd_fwd (F2)", B["wino2_in"],
         lambda s: cdiv(cdiv(s[0], 2) * cdiv(s[1], 2) * (s[2] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0,
         case="conv_f2_in"),
    _row("winograd_out_kernel", "winograd.hip:486", "strotss_conv3x3_winograd_fwd (F2)", B["wino2_out"],
         lambda s: cdiv(cdiv(s[0], 2) * cdiv(s[1], 2) * (s[3] // 4), 256), lambda s: s[2] % 32 == 0 and s[3] % 64 == 0,
         case="conv_f2_out"),
    _row("conv_splitk_finish_pool_kernel (x)", "conv.hip:497", "strotss_conv3x3_relu_pool_fwd", B["splitk_finish_pool_x"],
         lambda s: cdiv((s[1] // 2 + s[1] % 2) * (s[3] // 4), 256), lambda s: cdiv(s[0] * s[1], 64) * (s[3] // 64) <= 128,
         case="splitk_pool", named=False),
    _row("conv_splitk_finish_unpool_kernel (x)", "conv.hip:504", "strotss_conv3x3_dgrad_unpool", B["splitk_finish_unpool_x"],
         lambda s: cdiv((s[1] // 2 + s[1] % 2) * (s[3] // 4), 256), lambda s: cdiv((s[0] // 2) * (s[1] // 2), 64) * (s[3] // 64) <= 128,
         case="splitk_unpool", named=False),
    # ---- the panel split, the Sinkhorn kernel matrix and the centring of the f32 moment form
    _row("x3_split_rows_kernel", "gemm.hip:436", "strotss_conv3x3_winograd_x3pack", B["x3_split_rows"],
         lambda s: cdiv(s[0] * (s[1] // 4), 256), lambda s: s[0] > 0 and s[1] % 32 == 0, case="x3_split"),
    _row("sk_exp_kernel", "losses.hip:1466", "strotss_sinkhorn_cos_fwd_bwd", B["sk_exp"],
         lambda s: cdiv(s[0] * cdiv(s[1], 32) * 32, 256), lambda s: min(s) > 0, case="sk_exp"),
    _row("center_kernel", "losses.hip:1767, 1793", "strotss_moment_stats, strotss_moment_fwd_bwd (f32 GEMM form)",
         B["center_stats"], lambda s: cdiv(cdiv(s[0], 32) * 32 * cdiv(s[1], 32) * 32 // 4, 256), lambda s: min(s) > 0,
         case="center"),
]
# conv_splitk_finish_kernel (conv.hip:509, cap 2048 workgroups of 256 float4): conv_splits admits a layer only up to 128 tiles
# of 64 x 64 outputs, 128 x 4096 / 4 = 131072 float4 = 512 workgroups -- this cap can not be passed; the CPU file proves it.
UNREACHABLE = [("conv_splitk_finish_kernel", "conv.hip:509", B["splitk_finish"], 128 * 64 * 64 // 4 // 256)]


def rows_of(case):
    return [r for r in ROWS if r["case"] == case]


# ------------------------------------------------------------------ 3. the cases
def worst(err, allowed):
    """the largest err / allowed over the elements (0 / 0 counts as 0, anything that is not a number as inf)"""
    err, allowed = np.asarray(err, np.float64), np.broadcast_to(np.asarray(allowed, np.float64), np.shape(err))
    if err.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where((err == 0) & (allowed == 0), 0.0, err / allowed)
    return float(np.where(np.isnan(ratio), np.inf, ratio).max())


def judge_bounded(got, ref, bound, walked, what):
    """-> (figures, failures): every element finite and within its bound, over the whole output and over the walked region"""
    got = np.asarray(got, np.float64)
    assert got.shape == ref.shape and walked.shape == ref.shape[:walked.ndim], (what, got.shape, ref.shape, walked.shape)
    bound = np.broadcast_to(bound, ref.shape)
    err = np.abs(got - ref)
    fig = {f"{what}": worst(err, bound), f"{what} walked": worst(err[walked], bound[walked]),
           f"{what} unwritten": int((~np.isfinite(got)).sum())}
    bad = []
    if fig[f"{what} unwritten"]:
        bad.append(f"{what}: {fig[f'{what} unwritten']} elements are not finite (never written?)")
    if not fig[what] <= 1.0:
        bad.append(f"{what}: off by {fig[what]:.3g} of its bound")
    if not fig[f"{what} walked"] <= 1.0:
        bad.append(f"{what}: off by {fig[f'{what} walked']:.3g} of its bound in the walked region")
    assert walked.any(), f"{what}: the walked region is empty"
    return fig, bad


def judge_bits(got, ref, walked, what):
    """bit for bit, over the whole output and over the walked region"""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    view = {4: np.uint32, 2: np.uint16, 1: np.uint8, 8: np.uint64}[got.dtype.itemsize]
    differ = got.view(view) != ref.view(view)
    fig = {f"{what} bits": int(differ.sum()), f"{what} bits walked": int(differ[walked].sum())}
    assert walked.any(), f"{what}: the walked region is empty"
    bad = [f"{what}: {n} elements differ in their bits{where}" for n, where in
           ((fig[f"{what} bits"], ""), (fig[f"{what} bits walked"], " in the walked region")) if n]
    return fig, bad


def plant(ref, walked, fill):
    """the reference as the output would hold it after a walk that stops: walked elements keep `fill`"""
    out = np.array(ref, copy=True)
    out[walked] = fill[walked] if isinstance(fill, np.ndarray) else fill
    return out


_cache = {}


def once(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- guided_smooth.  The float64 restatement and E_round + E_stat of tests/_smooth_ref.py.  The strip is compared everywhere;
# at the wide shape (3.4 M pixels: 21 float64 planes and the budgets' 3 x 3 fields would take gigabytes) the restatement is
# taken on bands of rows -- the filter is local: a row's result depends on the rows within 2 r of it, so a band is computed from
# its rows and 2 r more on each side, exactly -- at the first rows, around the first walked row tile, around the first walked
# column tile and at the last rows; every other element must be finite over a NaN pre-fill.
SMOOTH_RADII = (1, 64)
SMOOTH_BAND_EVERY = 512
SMOOTH_CROP_ROWS = 3000                       # rows of an unwalked launch the GPU file compares the wide shape with, run by run
SMOOTH_EPS = 1e-2
SMOOTH_CASES = [(SMOOTH_STRIP, r) for r in SMOOTH_RADII] + [(SMOOTH_WIDE, r) for r in SMOOTH_RADII]


def smooth_walked(h, w):
    """pixels of the row tiles and of the column tiles from SMOOTH_MAX_GRID on"""
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    rows = y * cdiv(w, D["SMOOTH_ROW_THREADS"]) + x // D["SMOOTH_ROW_THREADS"] >= D["SMOOTH_MAX_GRID"]
    cols = (y // D["SMOOTH_COLS_Y"]) * cdiv(w, D["SMOOTH_COLS_X"]) + x // D["SMOOTH_COLS_X"] >= D["SMOOTH_MAX_GRID"]
    return rows | cols, rows, cols


def smooth_bands(h, w):
    """[(y0, y1)]: all rows of the strip; at the wide shape the walk edges, the ends and 8 rows in every SMOOTH_BAND_EVERY"""
    if h * w <= 2 ** 18:
        return [(0, h)]
    _, rows, cols = smooth_walked(h, w)
    yr, yc = int(np.argmax(rows.any(axis=1))), int(np.argmax(cols.any(axis=1)))
    assert rows.any() and cols.any()
    spans = [(0, 8), (yr - 8, yr + 8), (max(yc - 8, 0), min(yc + 8, h)), (h - 8, h)] + \
        [(y, y + 8) for y in range(SMOOTH_BAND_EVERY, h - 8, SMOOTH_BAND_EVERY)]      # and 8 rows in every 512
    return [(max(a, 0), min(b, h)) for a, b in spans]


def smooth_images(h, w, r):
    import _smooth_ref as S
    return once(("smooth images", h, w, r), lambda: S.test_images(h, w, 1000 * r + h + w))


def smooth_want(h, w, r):
    """[(y0, y1, q (y1 - y0, w, 3), bound)] per band"""
    import _smooth_ref as S

    def make():
        p, I = smooth_images(h, w, r)
        out = []
        for y0, y1 in smooth_bands(h, w):
            a, b = max(0, y0 - 2 * r), min(h, y1 + 2 * r)
            ref = S.guided_separable(p[a:b], I[a:b], r, SMOOTH_EPS, full=True)
            e_round, e_stat = S.error_budgets(p[a:b], I[a:b], r, SMOOTH_EPS, ref)
            assert e_stat.max() <= e_round.max()
            out.append((y0, y1, ref["q"][y0 - a:y1 - a], (e_round + e_stat)[y0 - a:y1 - a]))
        return out
    return once(("smooth want", h, w, r), make)


def smooth_judge(h, w, r, got):
    got = np.asarray(got, np.float64)
    walked = smooth_walked(h, w)[0]
    fig, bad = {"unwritten": int((~np.isfinite(got)).sum())}, []
    if fig["unwritten"]:
        bad.append(f"{fig['unwritten']} elements are not finite (never written?)")
    seen_walked = False
    for y0, y1, q, bound in smooth_want(h, w, r):
        wk = np.broadcast_to(walked[y0:y1, :, None], q.shape)
        err = np.abs(got[y0:y1] - q)
        a, b = worst(err, bound), worst(err[wk], bound[wk])
        seen_walked |= bool(wk.any())
        fig[f"rows {y0}..{y1}"], fig[f"rows {y0}..{y1} walked"] = a, b
        if not a <= 1.0 or not b <= 1.0:
            bad.append(f"rows {y0}..{y1}: off by {a:.3g} of the bound ({b:.3g} in the walked region)")
    assert seen_walked
    return fig, bad


def smooth_walk_stops(h, w, r, which):
    """the restatement's image with the pixels of the walked row tiles (`rows`) left at the NaN pre-fill; `cols`: the walked
    column tiles never wrote their window sums -- what the row pass then reads there is whatever the workspace held, NaN here"""
    out = np.zeros((h, w, 3))
    for y0, y1, q, _ in smooth_want(h, w, r):
        out[y0:y1] = q
    _, rows, cols = smooth_walked(h, w)
    out[rows if which == "rows" else cols] = NAN
    return out


# ---- guided_upsample, low-resolution passes at the strip
UPS_MODES = ("guided", "residual")
UPS_RADII = SMOOTH_RADII


def ups_inputs(r):
    import _upsample_ref as R
    return once(("ups images", r), lambda: R.test_images(*UPS_LO, *UPS_HI, 1000 * r + UPS_LO[0] + UPS_HI[1]))


def ups_walked():
    """output rows that read a record of a low-resolution row whose row tile (w = 3: the row itself) is walked"""
    import _pixel_ref as PR
    lo, hi, _ = PR.axis_table(UPS_LO[0], UPS_HI[0])
    rows = (np.maximum(lo, hi) >= D["SMOOTH_MAX_GRID"] // cdiv(UPS_LO[1], D["SMOOTH_ROW_THREADS"]))
    return np.broadcast_to(rows[:, None], UPS_HI).copy()


def ups_want(r, mode):
    import _upsample_ref as R

    def make():
        p, I_lo, I_hi = ups_inputs(r)
        ref = once(("ups coeff", r), lambda: R.coefficients(p, I_lo, r, SMOOTH_EPS))
        want = R.upsample(p, I_lo, I_hi, r, SMOOTH_EPS, mode, ref=ref)
        e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, SMOOTH_EPS, mode, ref)
        assert e_stat.max() <= e_round.max()
        return want, e_round + e_stat
    return once(("ups want", r, mode), make)


def ups_judge(r, mode, got):
    want, bound = ups_want(r, mode)
    return judge_bounded(got, want, bound, ups_walked(), f"upsample r {r} {mode}")


# ---- resize and its adjoint: tests/_pixel_ref.py
def resize_data(case):
    import _pixel_cases as PC
    ih, iw, oh, ow, c = case
    return once(("resize x", case), lambda: (PC.image(ih, iw, c=c), PC.normal((oh, ow, c), "add", oh, ow, c)))


def resize_want(case, alpha, with_add):
    import _pixel_ref as PR
    ih, iw, oh, ow, c = case
    x, add = resize_data(case)
    ref, s = once(("resize ref", case), lambda: PR.resize(x, oh, ow))
    a = add if with_add else None
    return alpha * ref + (0.0 if a is None else a.astype(np.float64)), PR.resize_bound(s, a)


def rows_walked(shape, cap):
    out = np.zeros(shape, bool)
    out[cap:] = True
    return out


def resize_judge(case, alpha, with_add, got):
    want, bound = resize_want(case, alpha, with_add)
    return judge_bounded(got, want, bound, rows_walked(want.shape, B["resize_y"]), f"resize alpha {alpha} add {with_add}")


def adjoint_data(case):
    import _pixel_cases as PC
    ih, iw, oh, ow, c = case
    return once(("adjoint g", case), lambda: PC.normal((oh, ow, c), "adj", *case))


def adjoint_want(case):
    import _pixel_ref as PR
    ih, iw = case[:2]
    return once(("adjoint ref", case), lambda: PR.adjoint(adjoint_data(case), ih, iw))


def adjoint_judge(case, got):
    import _pixel_ref as PR
    ref, b, m = adjoint_want(case)
    fig, bad = judge_bounded(got, ref, PR.adjoint_bound(b, m), rows_walked(ref.shape, B["resize_adjoint_y"]), "adjoint")
    none = np.broadcast_to(m == 0, ref.shape)
    if none.any() and not PR.plus_zero(np.asarray(got, np.float32)[none]):
        bad.append("adjoint: a pixel without a contributing output is not +0.0")
    return fig, bad


# ---- max-pool beyond 16384 rows of workgroups: values, codes and both backward forms bit for bit (tests/_pixel_ref.py)
def pool_data():
    import _pixel_cases as PC
    import _pixel_ref as PR
    h, w, c = POOL_TALL

    def make():
        x = PC.pool_input(h, w, c)
        mx, code = PR.maxpool(x)
        gout = PC.normal((h // 2, w // 2, c), "poolg", h, w, c)
        return dict(x=x, mx=mx, code=code, gout=gout, gin=PR.maxpool_bwd(code, gout, h, w), base=PC.pool_base(h, w, c))
    return once("pool", make)


def pool_walked():
    """(pooled rows from 16384 on, input rows of the coded backward's workgroup rows from 16384 on)"""
    h, w, c = POOL_TALL
    return rows_walked((h // 2, w // 2, c), B["maxpool_fwd_y"]), rows_walked((h, w, c), 2 * B["maxpool_bwd_code_y"])


def pool_want():
    d = pool_data()
    return dict(out=d["mx"], code=d["code"], gin_code=d["gin"], acc_code=d["base"] + d["gin"])


POOL_FILL = dict(out=np.float32(NAN), code=np.uint8(255), gin_code=np.float32(NAN), acc_code=None)       # None: the base


def pool_judge(got):
    want, (wo, wi) = pool_want(), pool_walked()
    fig, bad = {}, []
    for name, walked in (("out", wo), ("code", wo), ("gin_code", wi), ("acc_code", wi)):
        f, b = judge_bits(got[name], want[name], walked, name)
        fig.update(f)
        bad += b
    return fig, bad


def pool_walk_stops():
    want, (wo, wi) = pool_want(), pool_walked()
    fill = dict(POOL_FILL, acc_code=pool_data()["base"])
    return {name: plant(want[name], wo if name in ("out", "code") else wi, fill[name]) for name in want}


# ---- color_stats: ten float64 sums.  A sum has no walked region of its own: the planted result is the sum of the first trip
COLOR_WEIGHTS = (None, "random")


def color_data(kind):
    h, w = COLOR_STATS_SHAPE

    def make():
        rng = np.random.default_rng(h * w + (kind is not None))
        x = rng.random((h, w, 3)).astype(np.float32)
        m = None
        if kind == "random":
            m = (rng.random((h, w)) < 0.5).astype(np.float32)
            m.reshape(-1)[[0, -1]] = 1.0                                   # the one walked pixel counts
        return x, m
    return once(("color", kind), make)


def color_want(kind, first_trip=False):
    import _color_ref as CR
    x, m = color_data(kind)
    n = D["COLOR_MAX_BLOCKS"] * D["COLOR_THREADS"] * 4 if first_trip else x.shape[0] * x.shape[1]
    xs = x.reshape(-1, 3)[:n]
    ms = None if m is None else m.reshape(-1)[:n]
    return once(("color sums", kind, first_trip), lambda: CR.sums64(xs[None], None if ms is None else ms[None], exact=True))


def color_judge(kind, got):
    """test_hip_color.py's bound: N 2^-53 |ref| per sum (every term >= 0), and the count exact"""
    ref = color_want(kind)
    x, m = color_data(kind)
    n = x.shape[0] * x.shape[1]
    got = np.asarray(got, np.float64)
    fig = {"sums": worst(np.abs(got - ref), n * 2.0 ** -53 * np.abs(ref)), "count": float(got[0])}
    bad = []
    if not fig["sums"] <= 1.0:
        bad.append(f"sums off by {fig['sums']:.3g} of their bound")
    if got[0] != (n if m is None else float(m.sum())):
        bad.append(f"W = {got[0]!r}")
    return fig, bad


# ---- relu_bits: sign words bit for bit
def relu_bits_data():
    h, w, c = RELU_BITS_SHAPE
    return once("relu act", lambda: np.random.default_rng(h + w + c).standard_normal((h, w, c)).astype(np.float32))


def relu_bits_want():
    """(words (tiles, c) int32, the bits that lie inside the image)"""
    h, w, c = RELU_BITS_SHAPE

    def make():
        act = relu_bits_data()
        th, tw = cdiv(h, 4), cdiv(w, 4)
        pos = np.zeros((th * 4, tw * 4, c), bool)
        pos[:h, :w] = act > 0
        words = np.zeros((th * tw, c), np.int64)
        for r in range(4):
            for q in range(4):
                words |= pos[r::4, q::4].reshape(th * tw, c).astype(np.int64) << (8 * r + q)
        return words.astype(np.uint32).view(np.int32)
    return once("relu words", make)


def relu_bits_walked():
    words = relu_bits_want()
    flat = np.arange(words.size).reshape(words.shape)
    return flat >= B["relu_bits"] * 256


def relu_bits_judge(got):
    """the kernel writes 0 for the bits outside the image, as the restatement does: whole words are compared"""
    return judge_bits(np.asarray(got, np.int32), relu_bits_want(), relu_bits_walked(), "sign words")


# ---- winograd_weights on integer kernels: U = (24 G) k (24 G)^T / 576 exactly (tests/_exact_cases.py, condition 1)
WEIGHTS_TILES = (2, 4)


def weights_data():
    n, k = WEIGHTS_SHAPE
    return once("weights g", lambda: np.random.default_rng(n + k).integers(-3, 4, size=(n, k, 3, 3)).astype(np.float32))


def weights_want(tile):
    import _exact_cases as E

    def make():
        G = np.array(E.MATS[tile][2], np.float64)                          # 24 G, integers
        # an integer below 2^24 over 576: the correctly rounded double, then the one rounding to float32 the kernel has
        u = np.einsum("ar,nkrq,bq->abnk", G, weights_data().astype(np.float64), G) / 576.0
        return u.reshape((tile + 2) ** 2, *WEIGHTS_SHAPE).astype(np.float32)
    return once(("weights u", tile), make)


def weights_walked(tile):
    n, k = WEIGHTS_SHAPE
    flat = np.arange(n * k).reshape(n, k) >= B["winograd_weights"] * 256
    return np.broadcast_to(flat, ((tile + 2) ** 2, n, k))


def weights_judge(tile, got):
    return judge_bits(np.asarray(got, np.float32), weights_want(tile), weights_walked(tile), f"U F{tile}")


# ---- kmeans_assign_prior beyond 2048 tiles: tests/_track_ref.py's case and reference, _mask_edge_cases' comparison
ASSIGN_BETA = 0.05


def assign_want():
    import _track_ref as TR
    n, d, k = ASSIGN_PRIOR_SHAPE

    def make():
        x, inv, c32, prior = TR.assign_case(n, d, k)
        label, best, second, _, score = TR.assign_prior(x, inv, n, d, c32, prior, ASSIGN_BETA)
        return (x, inv, c32, prior), (label, best, second, score)
    return once("assign", make)


def assign_judge(got):
    import _mask_edge_cases as M
    n, d, k = ASSIGN_PRIOR_SHAPE
    _, ref = assign_want()
    first = D["KM_MAX_GRID"] * KM_TILE_ROWS
    fig, bad = {}, []
    for name, sl in (("", slice(0, n)), (" walked", slice(first, n))):
        f = M.assign_figures(tuple(np.asarray(g)[sl] for g in got), tuple(r[sl] for r in ref), d)
        fig.update({key + name: v for key, v in f.items()})
        bad += [b + name for b in M.assign_failures(f)]
    labels = np.asarray(got[0])
    if not ((labels >= 0) & (labels < k)).all():
        bad.append("labels outside 0..k-1 (never written?)")
    return fig, bad


def assign_walk_stops():
    _, (label, best, second, _) = assign_want()
    first = D["KM_MAX_GRID"] * KM_TILE_ROWS
    walked = np.arange(label.size) >= first
    return plant(label, walked, np.int32(-77)), plant(best, walked, NAN), plant(second, walked, NAN)


# ---- detail_map past all three of its caps: tests/_detail_map_ref.py's case and tolerance (4 E32 + 1e-7)
DETAIL_PARAMS = (2.0, 0.25)


def detail_want():
    import _detail_map_ref as DR
    return once("detail", lambda: DR.case("random", DETAIL_SHAPE, DETAIL_PARAMS))


def detail_walked():
    h, w, _ = DETAIL_SHAPE
    y, x = np.arange(h)[:, None], np.arange(w)[None, :]
    cols = (y // D["DM_COLS_Y"]) * cdiv(w, D["DM_COLS_X"]) + x // D["DM_COLS_X"] >= D["DM_MAX_GRID"]
    rows = y * cdiv(w, D["DM_ROW_THREADS"]) + x // D["DM_ROW_THREADS"] >= D["DM_ROWS_MAX_GRID"]
    scale = (y * w + x) // 4 >= D["DM_SCALE_MAX_GRID"] * D["DM_SCALE_THREADS"]
    return cols, rows, scale


def detail_judge(got):
    _, ref, _, e32 = detail_want()
    got = np.asarray(got, np.float64)
    bound = 4.0 * e32 + 1e-7
    fig, bad = {}, []
    for name, walked in zip(("column", "row", "scale"), detail_walked()):
        f, b = judge_bounded(got, ref, bound, walked, f"detail map, {name} walk")
        fig.update(f)
        bad += b
    lo = np.float32(DETAIL_PARAMS[1])
    if not (np.isfinite(got).all() and got.min() >= lo and got.max() <= 1.0):
        bad.append("levels outside [floor, 1]")
    return fig, bad


def detail_walk_stops(which):
    """column: the walked column tiles' plane is never written, their pixels come out as NaN; row: the walked row tiles never
    write `out` (NaN pre-fill); scale: the walked groups keep the unscaled local detail -- here the level before the division
    by the mean, which differs from the level wherever the mean is not 1"""
    import _detail_map_ref as DR
    img, ref, _, _ = detail_want()
    cols, rows, scale = detail_walked()
    if which == "scale":
        raw = DR.local_detail(img, DETAIL_SHAPE[2])
        return plant(ref, scale, raw)
    return plant(ref, cols if which == "column" else rows, NAN)


# ---- the convolution rows.  Integer data of tests/_exact_cases.py (every route's float32 result is the float64 one, bit
# for bit, under its conditions 2 .. 5, which the worker asserts on the sampled rows).  A whole float64 convolution of these
# sizes is too slow, so the reference is taken on SAMPLED TILE ROWS: the first tile row, the one before and the one of the first walked tile
# (work item cap x 256: tile cap x 256 / (channels / 4)), the last one and twelve seeded random ones -- at these smallest shapes the first walked tile lies in the LAST tile row,
# so the fixed rows are three and the sample is 15 x 182 tiles of 16
# pixels, every output channel -- and the whole output, pre-filled with NaN, must be finite.  name -> (switch group, tile,
# (h, w, cin, cout), which transform walks).  The groups run in a fresh child process each (the switches are read once).
CONV_GROUPS = {
    "default": {},
    "f32_gemms": {"STROTSS_X3": "0", "STROTSS_WINO_FUSED": "0"},
    "x3_panels": {"STROTSS_X3_CONV_F32A": "0"},
}
CONV_CASES = {
    "conv_in_f32": ("f32_gemms", 4, (724, 728, 512, 64), "in", 2),          # last: STROTSS_ROUTE_* the library must answer
    "conv_out": ("f32_gemms", 4, (724, 728, 64, 512), "out", 2),
    "conv_in_x3": ("x3_panels", 4, (724, 728, 512, 256), "in", 3),
    "conv_in_f32k": ("default", 4, (724, 728, 512, 256), "in", 3),
    "conv_f2_in": ("default", 2, (362, 364, 512, 64), "in", 0),
    "conv_f2_out": ("default", 2, (362, 364, 64, 512), "out", 0),
}
CONV_RANDOM_ROWS = 12
SPLITK_POOL_SHAPE = (2, 512, 64, 512)        # 128 tiles of 64 x 64, two K splits; 256 x 128 pooled float4 per row > 64 x 256
SPLITK_UNPOOL_SHAPE = (4, 1024, 64, 512)     # the (H, W) in front of the pool, over a 2 x 512 x 64 gradient; cin = 512


def conv_first_walked_tile(name):
    _, tile, (h, w, cin, cout), which, _ = CONV_CASES[name]
    c4 = (cin if which == "in" else cout) // 4
    return B["wino43_in"] * 256 // c4                                       # every transform cap is 16384 workgroups of 256


def conv_tile_rows(name):
    """the sampled tile rows, ascending"""
    _, tile, (h, w, _, _), _, _ = CONV_CASES[name]
    th, tw = cdiv(h, tile), cdiv(w, tile)
    ty = conv_first_walked_tile(name) // tw
    assert 1 <= ty <= th - 1, (name, ty, th)
    rng = np.random.default_rng(sum(map(ord, name)))
    fixed = {0, ty - 1, ty, min(ty + 1, th - 1), th - 1}        # (at the smallest shapes the walk begins in the last tile row)
    rest = [r for r in range(th) if r not in fixed]
    return sorted(fixed | set(rng.choice(rest, CONV_RANDOM_ROWS, replace=False).tolist()))


def conv_walked(name):
    """(len(rows) * tile, w) bool over the sampled image rows: pixels of the tiles from the first walked one on"""
    _, tile, (h, w, _, _), _, _ = CONV_CASES[name]
    tw = cdiv(w, tile)
    rows = np.array(conv_tile_rows(name))
    t = rows[:, None] * tw + np.arange(w)[None, :] // tile
    return np.repeat(t >= conv_first_walked_tile(name), tile, axis=0)


def conv_image_rows(name):
    """the image rows of the sampled tile rows (the last tile row may be cut by h)"""
    _, tile, (h, _, _, _), _, _ = CONV_CASES[name]
    y = (np.array(conv_tile_rows(name))[:, None] * tile + np.arange(tile)[None, :]).reshape(-1)
    return y, y < h


def conv_judge(name, got_rows, ref_rows, unwritten):
    """got_rows, ref_rows (sampled image rows, w, N) float32 / float64; unwritten: non-finite elements of the WHOLE output.
    Bit for bit on the sampled rows, over all of them and over the walked pixels alone"""
    y, inside = conv_image_rows(name)
    walked = conv_walked(name)[inside]
    got, ref = np.asarray(got_rows, np.float64)[inside], np.asarray(ref_rows, np.float64)[inside]
    differ = ~(got == ref)
    fig = {"unwritten": int(unwritten), "differ": int(differ.sum()), "differ walked": int(differ[walked].sum()),
           "sampled pixels": int(inside.sum() * got.shape[1]), "walked pixels": int(walked.sum())}
    assert walked.any() and not walked.all(), name
    bad = []
    if unwritten:
        bad.append(f"{unwritten} elements of the output are not finite (never written?)")
    if fig["differ"]:
        bad.append(f"{fig['differ']} sampled elements differ from float64 ({fig['differ walked']} in the walked region)")
    return fig, bad


def splitk_walked(shape, pooled):
    """pooled float4 index er = ox * (c / 4) + c4 >= 64 x 256 of a row: (w or w / 2, c) bool"""
    h, w, _, c = shape
    wo = w // 2
    er = np.arange(wo)[:, None] * (c // 4) + np.arange(c)[None, :] // 4
    m = er >= B["splitk_finish_pool_x"] * 256
    return m if pooled else np.repeat(m, 2, axis=0)


def splitk_pool_judge(got, want):
    """got, want: dict(out (h, w, c), pool, code (h / 2, w / 2, c)).  `out` is written by the thread of its pooled element"""
    fig, bad = {}, []
    for name, walked in (("out", splitk_walked(SPLITK_POOL_SHAPE, False)), ("pool", splitk_walked(SPLITK_POOL_SHAPE, True)),
                         ("code", splitk_walked(SPLITK_POOL_SHAPE, True))):
        f, b = judge_bits(got[name], want[name], np.broadcast_to(walked, want[name].shape), name)
        fig.update(f)
        bad += b
    return fig, bad


def splitk_unpool_judge(got, want):
    """got, want: dict(gin, acc (H, W, cin))"""
    H, W, _, cin = SPLITK_UNPOOL_SHAPE
    walked = np.broadcast_to(splitk_walked((H, W, 0, cin), False), (H, W, cin))
    fig, bad = {}, []
    for name in ("gin", "acc"):
        f, b = judge_bits(got[name], want[name], walked, name)
        fig.update(f)
        bad += b
    return fig, bad


# ---- x3_split_rows_kernel through strotss_conv3x3_winograd_x3pack: 36 x (rows, k) f32 -> panels (k / 32, 3 planes, rows, 32)
# bf16 (csrc/mfma_x3.h x3_store4), the planes h, m, l of split3 (tests/_exact_cases.py split3_t), bit for bit.  Work item
# e = ((kb rows + row) 8 + k4) of a batch: walked from kb rows + row >= 2048 x 256 / 8 on.
X3_SPLIT_SHAPE = (4128, 512)                  # rows k / 4 = 2^19 + 4096 work items a batch


def x3_panels(u):
    """u (batch, rows, k) float32 torch tensor -> (batch, k / 32, 3, rows, 32) bfloat16"""
    import torch
    import _exact_cases as E
    b, rows, k = u.shape
    planes = torch.stack([p.bfloat16() for p in E.split3_t(u)], 1)               # (b, 3, rows, k), each plane exact in bf16
    return planes.reshape(b, 3, rows, k // 32, 32).permute(0, 3, 1, 2, 4).contiguous()


def x3_walked():
    rows, k = X3_SPLIT_SHAPE
    item = np.arange(k // 32)[:, None] * rows + np.arange(rows)[None, :]
    return np.broadcast_to((item >= B["x3_split_rows"] * 256 // 8)[:, None, :, None], (k // 32, 3, rows, 32))


def x3_judge(got, ref):
    """got, ref: (batch, k / 32, 3, rows, 32) int16 views of the panels (NumPy)"""
    got, ref = np.asarray(got), np.asarray(ref)
    return judge_bits(got, ref, np.broadcast_to(x3_walked(), ref.shape), "x3 panels")


# ---- sk_exp_kernel through strotss_sinkhorn_cos_fwd_bwd: K = exp(-l M) over n x ldm entries, pred-major; past 4096 x 256
# entries the prediction rows from 2^20 / ldm on are walked.  Reference and tolerance: tests/_sinkhorn_ref.py (float64 autograd
# of the oracle; TOL_SK of the cosine family times max |ref|), data by tests/_sinkhorn_cases.py's generator.
SK_SHAPE = (1025, 1024, 35, 3)                # n, ns, d, T: n ldm = 1025 x 1024
SK_L = 10.0


def sk_case():
    import _sinkhorn_cases as SC

    def make():
        n, ns, d, T = SK_SHAPE
        rng = np.random.default_rng(n + ns + d)
        return SC.Case("launch_caps_n1025_ns1024", n, ns, d, T, "plain", ("cosine",), SC._rows(rng, ns, d), SC._rows(rng, n, d))
    return once("sk case", make)


def sk_want():
    import _sinkhorn_ref as SR
    c = sk_case()
    return once("sk want", lambda: SR.sinkhorn(c.x, c.y, "cosine", SK_L, c.T))


def sk_walked_rows():
    n, ns, _, _ = SK_SHAPE
    return np.arange(n) >= B["sk_exp"] * 256 // (cdiv(ns, 32) * 32)


def sk_judge(loss, grad):
    """the checks of test_hip_sinkhorn.py: the loss within loss_tolerance relative, every gradient element within TOL_SK of
    max |ref| -- over all rows and over the walked rows alone"""
    import _sinkhorn_ref as SR
    c = sk_case()
    ref_l, ref_g = sk_want()
    tol = SR.TOL_SK[SR.family(c, "cosine")] * np.abs(ref_g).max()
    grad = np.asarray(grad, np.float64)
    wk = sk_walked_rows()
    fig = {"loss": abs(loss - ref_l) / (SR.loss_tolerance(c, SK_L) * abs(ref_l)), "grad": worst(np.abs(grad - ref_g), tol),
           "grad walked": worst(np.abs(grad - ref_g)[wk], tol)}
    assert wk.any() and not wk.all()
    return fig, [f"{k}: off by {v:.3g} of its tolerance" for k, v in fig.items() if not v <= 1.0]


# ---- center_kernel (the moment term's f32 GEMM form, STROTSS_X3_MOMENT=0, a child process): cy = y - mean over rows x ld / 4
# float4; past 2048 x 256 of them the rows from 2^21 / ld on are walked.  References and bounds: tests/_loss_ref.py
# (moment_stats within cov_tau; moment's loss within TOL_SCALAR, its gradient by check_grad), on tests/_loss_cases.py's step case.
CENTER_LABEL = "step"
CENTER_SHAPE = (1024, 2179)
CENTER_ENV = {"STROTSS_X3_MOMENT": "0"}


def center_first_walked_row():
    n, d = CENTER_SHAPE
    return cdiv(B["center_stats"] * 256 * 4, cdiv(d, 32) * 32)          # the first row that is walked as a whole


def center_stats_judge(mean, cov, x):
    """strotss_moment_stats: |f32 - f64| <= cov_tau, entry by entry.  A covariance entry sums over every row: it has no walked
    region; the planted covariance lacks the walked rows' terms"""
    import _loss_ref as LR
    m64, S64 = once("center stats", lambda: LR.moment_stats(x))
    tc, tm = once("center tau", lambda: LR.cov_tau(x))
    fig = {"cov": worst(np.abs(np.asarray(cov, np.float64) - S64), tc), "mean": worst(np.abs(np.asarray(mean, np.float64) - m64), tm)}
    return fig, [f"{k}: off by {v:.3g} of cov_tau" for k, v in fig.items() if not v <= 1.0]


def center_grad_judge(loss, grad, x, y):
    """strotss_moment_fwd_bwd: test_hip_loss_terms.py's checks, over all rows and over the walked rows alone"""
    import _loss_ref as LR
    l, g, b, _ = once("center moment", lambda: LR.moment(x, y))
    r0 = center_first_walked_row()
    fig, bad = {"loss": abs(loss - l) / (LR.TOL_SCALAR * abs(l))}, []
    if not fig["loss"] <= 1.0:
        bad.append(f"loss off by {fig['loss']:.3g} of TOL_SCALAR")
    grad = np.asarray(grad, np.float64)
    scale = np.abs(g).max()                                             # check_grad's scale: max |ref| of the whole gradient
    for name, sl in (("grad", slice(None)), ("grad walked", slice(r0, None))):
        allowed = b[sl] + LR.TOL_GRAD * scale
        fig[name] = worst(np.abs(grad[sl] - g[sl]), allowed)
        if not fig[name] <= 1.0:
            bad.append(f"{name}: off by {fig[name]:.3g} of bound + TOL_GRAD max|ref|")
    ok, _, _ = LR.check_grad(grad, g, b, LR.TOL_GRAD)
    if not ok:
        bad.append("check_grad fails")
    return fig, bad


# ------------------------------------------------------------------ 4. the table of DESIGN.md
def _shape_text(s):
    return " x ".join(str(v) for v in s) if isinstance(s, tuple) and all(isinstance(v, int) for v in s) else str(s)


CASE_SHAPES = {
    "smooth": [SMOOTH_STRIP, SMOOTH_WIDE], "upsample": [UPS_LO], "maxpool_tall": [POOL_TALL], "resize": RESIZE_CASES,
    "resize_adjoint": ADJOINT_CASES, "color_stats": [COLOR_STATS_SHAPE], "relu_bits": [RELU_BITS_SHAPE],
    "winograd_weights": [WEIGHTS_SHAPE], "assign_prior": [ASSIGN_PRIOR_SHAPE], "detail_map": [DETAIL_SHAPE],
    "splitk_pool": [SPLITK_POOL_SHAPE], "splitk_unpool": [SPLITK_UNPOOL_SHAPE],
    "x3_split": [X3_SPLIT_SHAPE], "sk_exp": [SK_SHAPE[:2]], "center": [CENTER_SHAPE],
}
CASE_SHAPES.update({name: [c[2]] for name, c in CONV_CASES.items()})


def design_table():
    """kernel, launch, cap (workgroups, or rows of workgroups), a shape past it with the workgroups it asks for, the test"""
    lines = ["| kernel | launch | cap | a shape past it (workgroups wanted) | covered by |", "|---|---|---|---|---|"]
    for r in ROWS:
        if r["covered_by"]:
            shape, cover = r["covered_by"][4], f"`{r['covered_by'][0]}`"
        else:
            shape, cover = CASE_SHAPES[r["case"]][0], f"`test_hip_launch_caps` ({r['case']})"
        lines.append(f"| `{r['kernel']}` | {r['source']} | {r['cap']} | {_shape_text(shape)} ({r['work'](shape)}) | {cover} |")
    for kernel, source, cap, most in UNREACHABLE:
        lines.append(f"| `{kernel}` | {source} | {cap} | none: {most} at most | proved in `test_launch_caps_cpu` |")
    return "\n".join(lines)
