"""CPU: the exact-arithmetic cases of tests/_exact_cases.py meet their conditions, float32 stand-ins of every pipeline give
the float64 reference's bits on them, and planted errors fail the comparison functions tests/test_hip_exact_conv.py uses.

Conditions 2 .. 7 are checked per case on a seeded subset of tile rows (first, last, three drawn) over all tile columns and
channels -- the GPU file asserts them over everything -- and the float64 Winograd form on those rows must be the float64
convolution.  The stand-ins (numpy float32: direct, F(2x2,3x3), F(4x4,3x3) on an f32 chain, F(4x4,3x3) on the six split3
products) run on the bottom-right crop of each case, which keeps the case's partial tiles and all its channels."""
import numpy as np
import pytest
import torch

import _exact_cases as E
import _route_cases as RC

F32 = np.float32
ALL_INT_CASES = E.DEFAULT_CASES + [c for g in sorted(E.SWITCH_CASES) for c in E.SWITCH_CASES[g][1]]


# ------------------------------------------------------------------------------------------------ numpy stand-ins
def bf16_np(x):
    """float32 -> nearest bfloat16 (ties to even), kept as float32."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return ((b + (((b >> 16) & 1) + np.uint32(0x7FFF))) & np.uint32(0xFFFF0000)).view(F32)


def split3_np(x):
    h = bf16_np(x)
    r1 = (x - h).astype(F32)
    m = bf16_np(r1)
    r2 = (r1 - m).astype(F32)
    return [h, m, bf16_np(r2)]


PRODUCTS = [(2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)]       # (V plane, U plane) in the main loop's order: lh hl mm mh hm hh


def out_rows(m, tile):
    """A^T applied along axis 0 of m (P, ...) in the kernels' operation sequence, float32."""
    if tile == 2:
        return [m[0] + m[1] + m[2], m[1] - m[2] - m[3]]
    two, four, eight = F32(2), F32(4), F32(8)
    return [m[0] + m[1] + m[2] + m[3] + m[4], m[1] - m[2] + two * m[3] - two * m[4], m[1] + m[2] + four * m[3] + four * m[4],
            m[1] - m[2] + eight * m[3] - eight * m[4] + m[5]]


def standin(p, plant=None):
    """float32 stand-in of problem p's pipeline on the whole of p.a: the pre-activation (h, w, N) (bias added, no ReLU)."""
    plant = plant or {}
    a = p.a[0].numpy().astype(F32)
    bias = p.bias.numpy().astype(F32) if p.bias is not None else F32(0)
    if p.tile == 0:
        ap = np.pad(a, ((1, 1), (1, 1), (0, 0)))
        g = (576.0 * p.k_eff).numpy().astype(F32)
        out = np.zeros((p.h, p.w, p.N), dtype=F32)
        for r in range(3):
            for q in range(3):
                out += np.matmul(ap[r:r + p.h, q:q + p.w], g[r, q])
        return out + bias
    t = p.tile
    P = t + 2
    BT = np.array(E.MATS[t][0], dtype=F32)
    TH, TW = -(-p.h // t), -(-p.w // t)
    d = E.tile_patches(p.a[0], t, range(TH)).numpy().astype(F32)
    V = np.einsum("ar,rqtc,bq->abtc", BT, d, BT).reshape(P * P, TH * TW, p.K)
    assert V.dtype == F32
    U = E.kernel_u(p.k_eff, t).numpy().reshape(P * P, p.K, p.N)
    if "skip_kblock" in plant:                  # one 32-wide K-block of one tile never reaches the product
        tile_i, kb = plant["skip_kblock"]
        V = V.copy()
        V[:, tile_i, 32 * kb:32 * kb + 32] = 0
    if p.x3:
        Vs, Us = split3_np(V), split3_np(U)
        if plant.get("zero_v_plane") is not None:
            Vs[plant["zero_v_plane"]] = np.zeros_like(V)
        if plant.get("zero_u_plane") is not None:
            Us[plant["zero_u_plane"]] = np.zeros_like(U)
        M = np.zeros((P * P, TH * TW, p.N), dtype=F32)
        for pv, pu in PRODUCTS:
            if (pv, pu) not in plant.get("drop", ()):
                M = M + np.matmul(Vs[pv], Us[pu])
    else:
        M = np.matmul(V, U)
    assert M.dtype == F32
    M = M.reshape(P, P, TH * TW, p.N)
    s = out_rows(M, t)                                                    # s[i][q]
    y = [out_rows(np.stack([s[i][q] for q in range(P)]), t) for i in range(t)]      # y[i][j] (tiles, N), bias last
    Y = np.stack([np.stack([y[i][j] + bias for j in range(t)]) for i in range(t)]).astype(F32)
    return E.untile(torch.from_numpy(Y), p, range(TH))[:p.h].numpy()


def crop(p):
    """The bottom-right corner of problem p as a problem of its own: same channels and weights, the same h % 4 and w % 4."""
    hc = p.h if p.h <= 20 else 16 + p.h % 4
    wc = p.w if p.w <= 36 else 32 + p.w % 4
    q = E.Problem(p.id + ":crop", p.route, p.direction, hc, wc, p.cin, p.cout)
    q.a = p.a[:, p.h - hc:, p.w - wc:].contiguous()
    q.k_eff, q.bias = p.k_eff, p.bias
    if hasattr(p, "kind"):
        q.kind = p.kind
    return q


def seeded_rows(p):
    TH = -(-p.h // p.tile)
    rng = np.random.default_rng(E.zlib.crc32(p.id.encode()))
    return sorted({0, TH - 1} | set(int(v) for v in rng.integers(0, TH, 3)))


def conv64_rows(p, r0, r1):
    """Rows r0 .. r1 - 1 of the float64 convolution of p (without bias)."""
    lo, hi = max(r0 - 1, 0), min(r1 + 1, p.h)
    return E.conv64(p.a[:, lo:hi], 576.0 * p.k_eff)[:, r0 - lo:r1 - lo]


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_is_the_schedule_under_the_default_policy():
    assert not RC.misrouted(E.DEFAULT_CASES), RC.misrouted(E.DEFAULT_CASES)
    assert E.enumerate_default_cases() == E.DEFAULT_CASES
    keys = {E.class_key(c) for c in E.DEFAULT_CASES}
    assert len(keys) == len(E.DEFAULT_CASES)
    # no route, direction or remainder class the schedule's shapes produce is missing
    for h, w, cin, cout in E.schedule_layers():
        for direction in ("fwd", "dgrad"):
            c = (RC.route_of((None, direction, h, w, cin, cout)), direction, h, w, cin, cout)
            assert E.class_key(c) in keys, c
    assert {c[0] for c in E.DEFAULT_CASES} | {c[0] for g in E.SWITCH_CASES.values() for c in g[1]} == set(RC.ROUTES)
    for c in RC.DEFAULT_CASES:
        assert E.class_key(c) in keys, c
    print(len(E.DEFAULT_CASES), "default cases,", len(ALL_INT_CASES), "with the switch groups")


def test_split3_restatements_agree_and_are_exact():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.integers(-2 ** 24 + 1, 2 ** 24, 200000), rng.integers(-70000, 70000, 200000), [0, 1, -1, 65535, 65537,
                        2 ** 24 - 1, 255, 257, 383, 385]]).astype(F32)
    h, m, l = split3_np(x)
    th, tm, tl = E.split3_t(torch.from_numpy(x))
    assert np.array_equal(h, th.numpy()) and np.array_equal(m, tm.numpy()) and np.array_equal(l, tl.numpy())
    assert np.array_equal(h.astype(np.float64) + m + l, x.astype(np.float64))
    few = np.array([E.sig_bits(torch.tensor([float(v)], dtype=torch.float64)) for v in x[:2000]])
    assert np.all((l[:2000] == 0) | (few > 16)) and np.all((m[:2000] == 0) | (few > 8))
    assert E.sig_bits(torch.tensor([65537.0, 96.0], dtype=torch.float64)) == 17


@pytest.mark.parametrize("tile", [2, 4])
def test_the_weight_kernels_float64_sequence_gives_the_exact_integers(tile):
    """Condition 1 on the CPU: the kernel's sequence gives the integer (24 G) k (24 G)^T for sparse +-1 k, for 7-bit k over nine
    taps, and for every k in -1024 .. 1024 on a single tap -- also with the 1e-14 a contracted cancelling sum leaves on the
    device added to every entry, which only the zero test on the exact numerator removes."""
    g = E._gen(f"u-{tile}")
    for k in (torch.randint(-1, 2, (3, 3, 64, 128), generator=g).float(), torch.randint(-127, 128, (3, 3, 64, 128), generator=g).float()):
        assert torch.equal(E.kernel_u(k, tile).double(), E.exact_u(k, tile))
    k = torch.zeros(3, 3, 9, 2049)
    for t in range(9):
        k[t // 3, t % 3, t] = torch.arange(-1024, 1025).float()
    assert torch.equal(E.kernel_u(k, tile).double(), E.exact_u(k, tile))
    assert torch.equal(E.kernel_u(k, tile, residue=1e-14).double(), E.exact_u(k, tile))
    u = torch.from_numpy((E._gggt(E.G_DOUBLE[tile], 576.0 * k.double().numpy()) + 1e-14).astype(np.float32))
    assert not torch.equal(u.double(), E.exact_u(k, tile)), "without the zero test the residue survives"


# ------------------------------------------------------------------------------------------------ integer family
@pytest.mark.parametrize("case", ALL_INT_CASES, ids=E.case_id)
def test_integer_case_meets_its_conditions_and_the_standin_is_bit_for_bit(case):
    p = E.make_int_problem(case)
    extra = float(E.PRE_MAX) if p.direction == "dgrad" and p.route != "F2_gemm_f32" else 0.0
    if p.tile:
        rows = seeded_rows(p)
        fig, Y, _ = E.winograd_conditions(p, rows=rows, extra=extra)
        E.assert_winograd_conditions(fig, p.id)
        got = E.untile(Y, p, rows)
        ref = torch.cat([conv64_rows(p, r * p.tile, min((r + 1) * p.tile, p.h))[0] for r in rows])
        keep = torch.cat([torch.arange(r * p.tile, (r + 1) * p.tile) < p.h for r in rows])
        assert torch.equal(got[keep], ref), (p.id, "the float64 Winograd form is not the float64 convolution")
    else:
        lo = E.Problem(p.id, p.route, p.direction, min(p.h, 24), p.w, p.cin, p.cout)
        lo.a, lo.k_eff, lo.bias = p.a[:, :24], p.k_eff, p.bias
        fig = E.direct_conditions(lo, extra=extra)
        assert fig["sum"] < 1.0, (p.id, fig)
        ref = E.conv64(lo.a, 576.0 * p.k_eff)[0]
    pre = ref + (p.bias.double() if p.bias is not None else 0.0)
    fig["pos"], fig["neg"] = E.assert_nontrivial(pre, p.id)
    q = crop(p)
    if q.tile:
        figc, _, _ = E.winograd_conditions(q, extra=extra)
        E.assert_winograd_conditions(figc, q.id)
    want = E.conv64(q.a, 576.0 * q.k_eff) + (q.bias.double() if q.bias is not None else 0.0)
    got = torch.from_numpy(standin(q))[None]
    E.check_bitwise(got, want, q.id + " stand-in")
    print(f"{p.id:44s} " + " ".join(f"{k} {v:.3g}" for k, v in fig.items()))


def _small(route, direction, h, w, K=64, N=64):
    cin, cout = (K, N) if direction == "fwd" else (N, K)
    c = (route, direction, h, w, cin, cout)
    return E.make_int_problem(c)


def test_planted_skipped_k_block_of_a_tail_tile_fails():
    p = _small("F4_x3_gemm_64", "fwd", 13, 18)
    want = E.conv64(p.a, 576.0 * p.k_eff) + p.bias.double()
    E.check_bitwise(torch.from_numpy(standin(p))[None], want, "unplanted")
    last = (-(-13 // 4)) * (-(-18 // 4)) - 1
    with pytest.raises(AssertionError, match="not bit for bit"):
        E.check_bitwise(torch.from_numpy(standin(p, {"skip_kblock": (last, 1)}))[None], want, "planted")


def test_planted_partial_tile_column_from_its_neighbour_fails():
    p = _small("F4_gemm_f32", "fwd", 13, 18)
    want = torch.relu(E.conv64(p.a, 576.0 * p.k_eff) + p.bias.double())
    got = np.maximum(standin(p), 0)
    E.check_bitwise(torch.from_numpy(got)[None], want, "unplanted")
    got[:, 17] = got[:, 16]
    with pytest.raises(AssertionError, match="not bit for bit"):
        E.check_bitwise(torch.from_numpy(got)[None], want, "planted")


def test_planted_double_write_under_accumulate_fails():
    p = _small("F4_fused_f32", "dgrad", 13, 18)
    x = p.mask_input()
    base = p.base()
    v = standin(p) * (x[0].numpy() > 0)
    want = base.double() + E.conv64(p.a, 576.0 * p.k_eff) * (x > 0)
    got = base[0].numpy() + v
    E.check_bitwise(torch.from_numpy(got)[None], want, "unplanted")
    got[4:8, 4:8, 0:4] += v[4:8, 4:8, 0:4]
    assert np.any(v[4:8, 4:8, 0:4] != 0)
    with pytest.raises(AssertionError, match="not bit for bit"):
        E.check_bitwise(torch.from_numpy(got)[None], want, "planted")


def test_planted_sign_bit_at_a_zero_pre_activation_fails():
    p = _small("F4_fused_f32", "fwd", 13, 18)
    pre = E.conv64(p.a, 576.0 * p.k_eff) + p.bias.double()
    got = torch.from_numpy(standin(p))[None]
    E.check_bitwise(got, pre, "unplanted")
    zeros = (pre[0] == 0).nonzero()
    assert len(zeros) > 0, "no pre-activation is exactly 0"
    words = E.sign_words(got)[0]
    E.check_sign_words(words.int(), pre, "unplanted")
    y, x, c = (int(v) for v in zeros[0])
    words[(y // 4) * 5 + x // 4, c] ^= 1 << (8 * (y % 4) + x % 4)
    with pytest.raises(AssertionError, match="sign words differ"):
        E.check_sign_words(words.int(), pre, "planted")


def test_planted_last_maximum_pool_codes_fail():
    p = _small("F4_fused_f32", "fwd", 13, 18)
    pre = E.conv64(p.a, 576.0 * p.k_eff) + p.bias.double()
    assert E.tied_windows(pre) > 0, "no window with a tied positive maximum"
    pool, code = E.pool_reference(pre)
    want = torch.nn.functional.max_pool2d(torch.relu(pre).permute(0, 3, 1, 2), 2, 2).permute(0, 2, 3, 1)
    assert torch.equal(pool, want)
    E.check_codes(code, E.pool_reference(pre)[1], "unplanted")
    with pytest.raises(AssertionError, match="codes differ"):
        E.check_codes(E.pool_reference(pre, last=True)[1], code, "planted")


# ------------------------------------------------------------------------------------------------ wide family
LOOSENED = 2.0 ** 16          # the factor on WINO4_OUT_ROUNDINGS under which the planted plane errors pass


def _wide(kind, direction="fwd"):
    p = crop(E.make_wide_problem(E.WIDE_SHAPES[1], direction, kind))
    fig, Y, S = E.winograd_conditions(p)
    E.assert_winograd_conditions(fig, p.id, wide=True)
    rows = list(range(-(-p.h // 4)))
    bias = p.bias.double() if p.bias is not None else torch.zeros(1, dtype=torch.float64)
    ref = E.untile(Y, p, rows)[:p.h] + bias
    assert torch.equal(ref[None], E.conv64(p.a, 576.0 * p.k_eff) + bias)
    bound = E.GAMMA9 * (E.untile(S, p, rows)[:p.h] + bias.abs())
    return p, ref, bound


@pytest.mark.parametrize("shape", E.WIDE_SHAPES, ids=lambda s: f"{s[1]}-{s[2]}x{s[3]}x{s[4]}")
@pytest.mark.parametrize("direction", ["fwd", "dgrad"])
@pytest.mark.parametrize("kind", E.WIDE_KINDS)
def test_wide_case_meets_its_conditions_and_floors(shape, direction, kind):
    p = E.make_wide_problem(shape, direction, kind)
    rows = seeded_rows(p)
    fig, Y, _ = E.winograd_conditions(p, rows=rows)
    E.assert_winograd_conditions(fig, p.id, wide=True)
    sm, sl = E.plane_shares(p, rows)
    fm, fl = E.WIDE_FLOORS[kind]
    assert sm >= fm and sl >= fl, (p.id, sm, sl)
    keep = torch.cat([torch.arange(r * 4, r * 4 + 4) < p.h for r in rows])
    E.assert_nontrivial(E.untile(Y, p, rows)[keep] + (p.bias.double() if p.bias is not None else 0.0), p.id)
    print(f"{p.id:52s} sum|U||V| {fig['m']:.3f} out {fig['out']:.3f} bits V {fig['bits_v']} U {fig['bits_u']} m {sm:.3f} l {sl:.3f}")


@pytest.mark.parametrize("kind,plant", [("v12", {"zero_v_plane": 1}), ("v17", {"zero_v_plane": 1}), ("u17", {"zero_u_plane": 1}),
                                        ("v17", {"drop": ((2, 0),)})],
                         ids=["m_of_V_dropped_v12", "m_of_V_dropped_v17", "m_of_U_dropped", "lh_dropped_hl_kept"])
def test_planted_plane_errors_fail_under_the_derived_bound_and_pass_a_loosened_one(kind, plant):
    p, ref, bound = _wide(kind)
    clean = E.check_bound(torch.from_numpy(standin(p)), ref, bound, "unplanted")
    bad = torch.from_numpy(standin(p, plant))
    with pytest.raises(AssertionError, match="error / bound"):
        E.check_bound(bad, ref, bound, "planted")
    loose = E.check_bound(bad, ref, bound * LOOSENED, "planted, loosened")
    print(f"{kind} {plant}: unplanted {clean:.3f} of the bound, planted {loose * LOOSENED:.1f} of it")


# ------------------------------------------------------------------------------------------------ distance GEMM
@pytest.mark.parametrize("shape", E.DIST_SHAPES, ids=lambda s: s[0])
@pytest.mark.parametrize("kind", E.DIST_KINDS)
def test_distance_rows_meet_their_condition_and_the_standin_is_bit_for_bit(shape, kind):
    label, n, ns = shape
    x, y = E.make_dist_rows(label, n, ns, kind)
    s, (sm, sl) = E.dist_conditions(x, y)
    z = E.dist_self_operand(x, y, kind)
    sz = E.dist_conditions(z, z)[0]
    assert s < 1.0 and sz < 1.0, (label, kind, s, sz)
    if kind != "dense":
        assert sm >= 0.5 and (sl >= 0.1 or kind == "both_mid"), (label, kind, sm, sl)
    n_, ns_ = min(n, 96), min(ns, 96)
    xs, ys = split3_np(x[:n_].numpy()), split3_np(y[:ns_].numpy())
    acc = np.zeros((n_, ns_), dtype=F32)
    for px, py in PRODUCTS:
        acc = acc + np.matmul(xs[px], ys[py].T)
    got = (F32(1) - acc * F32(1)).astype(F32)
    E.check_bitwise(torch.from_numpy(got)[None], (1.0 - x[:n_].double() @ y[:ns_].double().T)[None], f"{label} {kind}")
    print(f"distance {label:14s} {kind:9s} sum {s:.3g} self {sz:.3g} of 2^24  m {sm:.3f} l {sl:.3f}")
