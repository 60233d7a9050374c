"""The inventory of capped launches (tests/_launch_cap_cases.py) checked on the host: every mirrored constant equals the source's,
every row's shape asks for more workgroups than its cap and lies inside its entry's argument ranges, every `covered_by` shape
is one the cited module really holds, every capped launch of csrc is a row, and for every new case the comparison that judges
the device's result rejects the result of a walk that stops after its first trip (and accepts the reference itself)."""
import importlib
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _launch_cap_cases as L  # noqa: E402

ROOT = L.ROOT


# ------------------------------------------------------------------ 1. the constants and the list
@pytest.mark.parametrize("name", sorted(L.DEFINES))
def test_mirrored_define_equals_the_source(name):
    assert L.define_in_source(name) == L.DEFINES[name][1]


@pytest.mark.parametrize("name", sorted(L.BARE))
def test_mirrored_bare_cap_equals_the_source(name):
    assert L.bare_in_source(name) == L.BARE[name][2]


def test_derived_constants():
    assert L.KM_TILE_ROWS == 32 and L.UPS_TILE == 1024
    text = open(os.path.join(L.CSRC, "kmeans_assign.h")).read()
    assert "#define KM_TILE_ROWS ((KM_ASSIGN_THREADS / WAVE) * KM_ROWS_PER_WAVE)" in text
    assert "#define UPS_TILE (UPS_THREADS * UPS_PIXELS)" in open(os.path.join(L.CSRC, "smooth.hip")).read()
    assert "#define COLOR_PIX_PER_BLOCK (4 * COLOR_THREADS)" in open(os.path.join(L.CSRC, "color.hip")).read()


def _capped_launch_lines():
    """(file, line number) of every launch in csrc whose grid holds a `min(`, a *_MAX_* constant or a `> n ? n :` cap -- on the
    launch's own line or on the line that declares the grid it names"""
    found = []
    cap = re.compile(r"\bmin\(|_MAX_(GRID|BLOCKS)\b|> \d+ \? \d+ :")
    grid = re.compile(r"hipLaunchKernelGGL|\bdim3 \w+\(|\bint nparts =")
    for name in sorted(os.listdir(L.CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        for i, line in enumerate(open(os.path.join(L.CSRC, name)).read().split("\n")):
            code = line.split("//")[0]
            if grid.search(code) and cap.search(code):
                found.append((name, i + 1))
    return found


def test_every_cap_constant_of_csrc_is_mirrored():
    names = set()
    for name in sorted(os.listdir(L.CSRC)):
        if name.endswith((".hip", ".h")):
            names |= set(re.findall(r"^#define (\w+_MAX_(?:GRID|BLOCKS|ROW_BLOCKS))\b", open(os.path.join(L.CSRC, name)).read(), re.M))
    assert names and names <= set(L.DEFINES), names - set(L.DEFINES)


def _launch_statement(lines, i):
    """the launch statement that uses the grid of line i: that line's own, or the next hipLaunchKernelGGL lines up to the
    end of the function (a `const dim3 grid(...)` may serve several launches)"""
    if "hipLaunchKernelGGL" in lines[i]:
        return lines[i] + (lines[i + 1] if i + 1 < len(lines) else "")
    out = []
    for line in lines[i + 1:i + 40]:
        if line.startswith("}"):
            break
        if "hipLaunchKernelGGL" in line:
            out.append(line)
    return " ".join(out)


def test_every_capped_launch_of_csrc_is_a_row():
    """every capped grid the scan finds feeds a launch of a kernel that some row (or the unreachable list) names; the caps
    inside helpers (stats_blocks, walk_blocks, row_blocks, dm_rows_grid) are found through test_every_cap_constant_..."""
    named = " ".join(r["kernel"] for r in L.ROWS) + " " + " ".join(u[0] for u in L.UNREACHABLE)
    names = set(re.findall(r"\w+_kernel\w*|\w+_kernel", named))
    missing = []
    for file, n in _capped_launch_lines():
        lines = open(os.path.join(L.CSRC, file)).read().split("\n")
        kernels = re.findall(r"hipLaunchKernelGGL\(\(?(\w+)", _launch_statement(lines, n - 1))
        assert kernels, (file, n, "a capped grid without a launch")
        missing += [(file, n, k) for k in kernels if k not in names and k != "calib_copy_kernel"]
    assert not missing, f"capped launches without a row: {missing}"
    # and every row's source names a line of its file that mentions a launch, a grid or the helper of one
    for r in L.ROWS:
        file, rest = r["source"].split(":", 1)
        lines = open(os.path.join(L.CSRC, file)).read().split("\n")
        for k in re.findall(r"\d+", rest):
            near = " ".join(lines[max(int(k) - 3, 0):int(k) + 2])
            assert re.search(r"hipLaunchKernelGGL|dim3|row_blocks|stats_blocks|walk_blocks", near), (r["kernel"], file, k)


# ------------------------------------------------------------------ 2. the rows
def _shapes_of(row):
    if row["covered_by"]:
        return [row["covered_by"][4]]
    return L.CASE_SHAPES[row["case"]]                      # upsample: the low-resolution size, whose passes the rows are


@pytest.mark.parametrize("row", L.ROWS, ids=lambda r: r["kernel"].split(",")[0].replace(" ", "_"))
def test_row_is_past_its_cap_and_inside_the_entrys_ranges(row):
    for shape in _shapes_of(row):
        work = row["work"](shape)
        assert work > row["cap"], (row["kernel"], shape, work, row["cap"])          # workgroups wanted > workgroups launched
        assert row["ok"](shape), (row["kernel"], shape, "outside the entry's documented ranges")


def test_the_split_k_finish_can_not_pass_its_cap():
    text = open(os.path.join(L.CSRC, "conv.hip")).read()
    assert "if (!on || tiles > 128) return 0;" in text and "cdiv((int64_t)H * W, 64) * (Cout / 64)" in text
    for _, _, cap, most in L.UNREACHABLE:
        assert most == 128 * 64 * 64 // 4 // 256 and most < cap


def _holds(container, shape):
    if isinstance(container, dict):
        return any(_holds(v, shape) for v in container.values())
    if isinstance(container, (list, tuple)) and container and container != shape:
        return any(v == shape or (isinstance(v, (list, tuple, dict)) and _holds(v, shape)) for v in container)
    return container == shape


def _parametrized_values(fn):
    """every value list of the function's own parametrize marks"""
    return [list(m.args[1]) for m in getattr(fn, "pytestmark", []) if m.name == "parametrize"]


@pytest.mark.parametrize("row", [r for r in L.ROWS if r["covered_by"]], ids=lambda r: r["kernel"].split(",")[0].replace(" ", "_"))
def test_covered_by_names_a_shape_its_test_runs(row):
    """the cited FUNCTION runs the shape: one of its parametrize marks holds the shape (or the key of the dict entry that
    holds it), or -- where the function loops itself -- its own source names the list, or writes the shape out"""
    import inspect
    test, module, attr, key, shape = row["covered_by"]
    assert "::" in test, test
    test_module = importlib.import_module(test.split("::")[0])
    fn = getattr(test_module, test.split("::")[1])
    body = inspect.getsource(fn)
    if attr is None:                                        # the shape is written in the body of the test
        assert re.search(r"\(%d, %d\)" % shape, body), (test, shape)
        return
    held = getattr(importlib.import_module(module), attr)
    values = _parametrized_values(fn)
    if isinstance(held, dict):
        assert key in held, (attr, key)
        entry = held[key][0] if attr == "REFINE_CASES" else held[key]
        assert entry[:len(shape)] == shape if attr == "REFINE_CASES" else _holds(entry, shape), (attr, key, shape)
        assert any(key in v for v in values), (test, "does not parametrise over", attr, key)
        return
    assert _holds(held, shape) or held == shape, (module, attr, shape)
    in_marks = any(_holds(v, shape) for v in values)
    in_body = re.search(r"\b%s\b" % attr, body) is not None
    assert in_marks or in_body, (test, "neither parametrises over nor names", attr)


def test_named_rows_of_the_issue_are_present():
    kernels = " ".join(r["kernel"] for r in L.ROWS) + " " + " ".join(u[0] for u in L.UNREACHABLE)
    for name in ("color_stats_kernel", "smooth_cols1_kernel", "smooth_cols2_kernel", "smooth_rows", "winograd43_in_kernel",
                 "winograd43_in_x3_kernel", "winograd43_in_f32k_kernel", "winograd43_out_kernel", "winograd_in_kernel",
                 "winograd_out_kernel", "relu_bits_kernel", "maxpool2_bwd_kernel", "maxpool2_fwd_kernel",
                 "maxpool2_bwd_code_kernel", "conv_splitk_finish_kernel", "conv3x3_c3_fwd_mfma_kernel", "x3_split_rows_kernel",
                 "sk_exp_kernel", "center_kernel", "winograd43_pack_kernel", "resize_bilinear_kernel", "resize_adjoint_kernel",
                 "refine_vote_kernel", "upsample_apply_kernel", "color_hist_kernel", "detail_cols_kernel", "detail_rows_kernel",
                 "detail_scale_kernel", "kmeans_assign_kernel", "kmeans_partial_kernel"):
        assert name in kernels, name


def test_design_table_is_generated_from_the_rows():
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert L.design_table() in text


# ------------------------------------------------------------------ 3. every new case sees a walk that stops
def _accepts(fig_bad):
    return not fig_bad[1]


def test_smooth_strip_rejects_a_walk_that_stops():
    (h, w), r = L.SMOOTH_STRIP, 1
    perfect = L.smooth_walk_stops(h, w, r, "rows")
    whole = np.concatenate([q for _, _, q, _ in L.smooth_want(h, w, r)])
    assert _accepts(L.smooth_judge(h, w, r, whole.astype(np.float32)))
    for which in ("rows", "cols"):
        fig, bad = L.smooth_judge(h, w, r, L.smooth_walk_stops(h, w, r, which))
        assert bad and fig["unwritten"] > 0, which
    assert np.isnan(perfect).any()


def test_smooth_wide_rejects_a_walk_that_stops():
    """on its bands: the planted image is the restatement on the bands, zeros elsewhere (finite: only the walk is planted)"""
    (h, w), r = L.SMOOTH_WIDE, 1
    _, rows, cols = L.smooth_walked(h, w)
    assert rows.any() and cols.any() and not rows.all() and not cols.all()
    assert w > L.D["SMOOTH_ROW_THREADS"]
    good = np.zeros((h, w, 3))
    for y0, y1, q, _ in L.smooth_want(h, w, r):
        good[y0:y1] = q
    assert _accepts(L.smooth_judge(h, w, r, good))
    for which in ("rows", "cols"):
        assert not _accepts(L.smooth_judge(h, w, r, L.smooth_walk_stops(h, w, r, which))), which


def test_upsample_rejects_a_walk_that_stops():
    r, mode = 1, "guided"
    want, _ = L.ups_want(r, mode)
    walked = L.ups_walked()
    assert walked.any() and not walked.all()
    assert _accepts(L.ups_judge(r, mode, want.astype(np.float32)))
    assert not _accepts(L.ups_judge(r, mode, L.plant(want, walked, L.NAN)))


@pytest.mark.parametrize("case", L.RESIZE_CASES, ids=str)
def test_resize_rejects_a_walk_that_stops(case):
    want, _ = L.resize_want(case, -1.0, True)
    walked = L.rows_walked(want.shape, L.B["resize_y"])
    assert _accepts(L.resize_judge(case, -1.0, True, want.astype(np.float32)))
    assert not _accepts(L.resize_judge(case, -1.0, True, L.plant(want, walked, L.NAN)))
    first_trip = want.copy()
    first_trip[L.B["resize_y"]:] = want[:want.shape[0] - L.B["resize_y"]]           # the rows one trip earlier
    assert not _accepts(L.resize_judge(case, -1.0, True, first_trip))


@pytest.mark.parametrize("case", L.ADJOINT_CASES, ids=str)
def test_resize_adjoint_rejects_a_walk_that_stops(case):
    ref, _, _ = L.adjoint_want(case)
    walked = L.rows_walked(ref.shape, L.B["resize_adjoint_y"])
    assert _accepts(L.adjoint_judge(case, ref.astype(np.float32)))
    assert not _accepts(L.adjoint_judge(case, L.plant(ref, walked, L.NAN)))


def test_maxpool_rejects_a_walk_that_stops():
    want = L.pool_want()
    assert _accepts(L.pool_judge(want))
    fig, bad = L.pool_judge(L.pool_walk_stops())
    assert len(bad) == 8 and all(fig[f"{k} bits walked"] == fig[f"{k} bits"] > 0 for k in want), (fig, bad)


@pytest.mark.parametrize("kind", L.COLOR_WEIGHTS, ids=str)
def test_color_stats_rejects_the_sum_of_the_first_trip(kind):
    assert _accepts(L.color_judge(kind, L.color_want(kind)))
    assert not _accepts(L.color_judge(kind, L.color_want(kind, first_trip=True)))
    h, w = L.COLOR_STATS_SHAPE
    assert (h * w) % 4 != 0 and h * w == L.D["COLOR_MAX_BLOCKS"] * L.D["COLOR_THREADS"] * 4 + 1       # the smallest such count


def test_relu_bits_rejects_a_walk_that_stops():
    words, walked = L.relu_bits_want(), L.relu_bits_walked()
    assert _accepts(L.relu_bits_judge(words))
    fig, bad = L.relu_bits_judge(L.plant(words, walked, np.int32(-1)))
    assert bad and fig["sign words bits walked"] == int(walked.sum())


@pytest.mark.parametrize("tile", L.WEIGHTS_TILES)
def test_winograd_weights_rejects_a_walk_that_stops(tile):
    u, walked = L.weights_want(tile), L.weights_walked(tile)
    assert _accepts(L.weights_judge(tile, u))
    assert not _accepts(L.weights_judge(tile, L.plant(u, walked, np.float32(L.NAN))))


def test_assign_prior_rejects_a_walk_that_stops():
    _, (label, best, second, _) = L.assign_want()
    assert _accepts(L.assign_judge((label, best.astype(np.float32), second.astype(np.float32))))
    assert not _accepts(L.assign_judge(L.assign_walk_stops()))


@pytest.mark.parametrize("which", ["column", "row", "scale"])
def test_detail_map_rejects_a_walk_that_stops(which):
    _, ref, _, _ = L.detail_want()
    assert _accepts(L.detail_judge(ref.astype(np.float32)))
    assert not _accepts(L.detail_judge(L.detail_walk_stops(which)))


@pytest.mark.parametrize("name", sorted(L.CONV_CASES))
def test_convolution_sample_sees_a_walk_that_stops(name):
    """the geometry of the real case (sampled tile rows, walked tiles) on a stand-in reference of the sampled rows' shape: the
    data of the 1 GB case is made on the device, the comparison and what it looks at are the ones used there"""
    group, tile, (h, w, cin, cout), which, _ = L.CONV_CASES[name]
    rows = L.conv_tile_rows(name)
    first = L.conv_first_walked_tile(name)
    tw = L.cdiv(w, tile)
    assert {0, first // tw, L.cdiv(h, tile) - 1} <= set(rows) and (first - 1) // tw in rows          # first, straddling, last
    assert len(rows) * tile * w >= 2048 + 4 * tile * tile
    assert first * ((cin if which == "in" else cout) // 4) == 16384 * 256
    ref = np.random.default_rng(1).integers(0, 50, size=(len(rows) * tile, w, 8)).astype(np.float64)
    assert _accepts(L.conv_judge(name, ref.astype(np.float32), ref, 0))
    walked = L.conv_walked(name)
    fig, bad = L.conv_judge(name, L.plant(ref, walked, L.NAN), ref, int(walked.sum()) * 8)
    assert bad and fig["differ walked"] == fig["differ"] > 0
    stale = ref.copy()
    stale[walked] = ref[~walked][:int(walked.sum())] + 1.0                  # the first trip's values, finite
    assert not _accepts(L.conv_judge(name, stale, ref, 0))


def test_conv_groups_name_real_switches():
    text = "".join(open(os.path.join(L.CSRC, f)).read() for f in ("winograd.hip", "winograd_fused.hip"))
    for env in L.CONV_GROUPS.values():
        for k in env:
            assert f'getenv("{k}")' in text, k


def test_splitk_finishes_reject_a_walk_that_stops():
    h, w, _, c = L.SPLITK_POOL_SHAPE
    rng = np.random.default_rng(2)
    want = dict(out=rng.random((h, w, c), dtype=np.float32), pool=rng.random((h // 2, w // 2, c), dtype=np.float32),
                code=rng.integers(0, 5, (h // 2, w // 2, c)).astype(np.uint8))
    assert _accepts(L.splitk_pool_judge(want, want))
    full, pooled = L.splitk_walked(L.SPLITK_POOL_SHAPE, False), L.splitk_walked(L.SPLITK_POOL_SHAPE, True)
    assert pooled.any() and not pooled.all()
    planted = dict(out=L.plant(want["out"], np.broadcast_to(full, want["out"].shape), np.float32(L.NAN)),
                   pool=L.plant(want["pool"], np.broadcast_to(pooled, want["pool"].shape), np.float32(L.NAN)),
                   code=L.plant(want["code"], np.broadcast_to(pooled, want["code"].shape), np.uint8(9)))
    assert len(L.splitk_pool_judge(planted, want)[1]) == 6
    H, W, _, cin = L.SPLITK_UNPOOL_SHAPE
    g = dict(gin=rng.random((H, W, cin), dtype=np.float32), acc=rng.random((H, W, cin), dtype=np.float32))
    assert _accepts(L.splitk_unpool_judge(g, g))
    wk = np.broadcast_to(L.splitk_walked((H, W, 0, cin), False), (H, W, cin))
    assert len(L.splitk_unpool_judge({k: L.plant(v, wk, np.float32(L.NAN)) for k, v in g.items()}, g)[1]) == 4


def test_x3_panel_split_rejects_a_walk_that_stops():
    """one batch of the 36 (the walk is per batch) through the comparison the GPU test uses; the layout restated against
    x3_store4's offset formula on a few elements"""
    import torch
    rows, k = L.X3_SPLIT_SHAPE
    u = torch.randn((1, rows, k), generator=torch.Generator().manual_seed(3))
    want = L.x3_panels(u)
    flat = want.reshape(-1).float()
    import _exact_cases as E
    planes = E.split3_t(u[0])
    for row, k0, pl in ((0, 0, 0), (rows - 1, k - 1, 2), (3617, 480 + 5, 1), (17, 33, 1)):
        o = ((k0 >> 5) * 3 * rows + row) * 32 + (k0 & 31) + pl * rows * 32          # csrc/mfma_x3.h x3_store4
        assert float(flat[o]) == float(planes[pl][row, k0])
    ref = want.view(torch.int16).numpy()
    walked = np.broadcast_to(L.x3_walked(), ref.shape)
    assert walked.any() and not walked.all()
    assert _accepts(L.x3_judge(ref, ref))
    assert not _accepts(L.x3_judge(L.plant(ref, walked, np.int16(0x7FC0)), ref))


def test_sinkhorn_case_rejects_a_walk_that_stops():
    """sk_exp's walked entries are the kernel matrix of the walked prediction rows: left at what the workspace held, those
    rows' gradient is not the reference's -- planted as zero (finite) and as NaN"""
    import _sinkhorn_ref as SR
    c = L.sk_case()
    assert SR.conditioned(c, "cosine", L.SK_L)
    ref_l, ref_g = L.sk_want()
    wk = L.sk_walked_rows()
    assert int(wk.sum()) == 1
    assert _accepts(L.sk_judge(ref_l, ref_g.astype(np.float32)))
    for fill in (0.0, L.NAN):
        g = ref_g.copy()
        g[wk] = fill
        assert not _accepts(L.sk_judge(ref_l, g)), fill


def test_center_case_rejects_a_walk_that_stops():
    """the centred rows from the first walked one on left at zero: the covariance lacks their terms, the gradient its rows"""
    import _loss_cases as LC
    import _loss_ref as LR
    c = LC.make_case(L.CENTER_LABEL)
    r0 = L.center_first_walked_row()
    assert 0 < r0 < c.n and L.cdiv(r0 * 2208 // 4, 256) >= 2048
    m, S = LR.moment_stats(c.x)
    assert _accepts(L.center_stats_judge(m.astype(np.float32), S.astype(np.float32), c.x))
    cx = c.x - m
    cx[r0:] = 0.0
    assert not _accepts(L.center_stats_judge(m, cx.T @ cx / c.ns, c.x))
    l, g, b, _ = LR.moment(c.x, c.y)
    assert _accepts(L.center_grad_judge(l, g.astype(np.float32), c.x, c.y))
    stale = g.copy()
    stale[r0:] = 0.0
    assert not _accepts(L.center_grad_judge(l, stale, c.x, c.y))
