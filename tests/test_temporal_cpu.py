"""Temporal consistency of frame sequences without a GPU: the --video / --flow_dir / --temporal_weight / --temporal_init
command line and its refusals, the .flo reader, the flow resize's vector scaling, the float64 restatement of the warp, the
certainty and L_t on hand cases, the warp's rule for out-of-range and non-finite coordinates, the conditions of the device
test's cases (every threshold test a margin away from equality), and the status codes of refused strotss_flow_warp /
strotss_temporal_fwd_bwd calls (checked before anything launches)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _temporal_ref as T  # noqa: E402

EINVAL, EALIGN = -1, -2
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)        # non-null, not 16-byte aligned


def _args(*extra, content="c.jpg"):
    import run_strotss as RS
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


def _sequence(tmp_path, n=3):
    frames, flows = tmp_path / "frames", tmp_path / "flows"
    T.translated_sequence(str(frames), str(flows), n_frames=n, h=12, w=16)
    return str(frames), str(flows)


# ------------------------------------------------------------------ command line
def test_video_flags_parse():
    a = _args("--video", "--flow_dir", "f", "--temporal_weight", "2.5", "--temporal_init", "-o", "out")
    assert a.video and a.flow_dir == "f" and a.temporal_weight == 2.5 and a.temporal_init and a.output_path == "out"
    a = _args()
    assert not a.video and a.flow_dir is None and a.temporal_weight is None and not a.temporal_init


def test_video_inputs_wiring(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert RS._video_inputs(_args()) is None
    frames, flows = _sequence(tmp_path)
    got, lam = RS._video_inputs(_args("--video", "--flow_dir", flows, content=frames))
    assert [os.path.basename(f) for f in got] == ["frame_01.png", "frame_02.png", "frame_03.png"]
    assert lam == RS.DEFAULT_TEMPORAL_WEIGHT > 0
    assert RS._video_inputs(_args("--video", "--flow_dir", flows, "--temporal_weight", "0", content=frames))[1] == 0.0
    assert RS._video_inputs(_args("--video", "--flow_dir", flows, "--temporal_weight", "7", content=frames))[1] == 7.0


def test_video_refusals(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames, flows = _sequence(tmp_path)
    ok = ("--video", "--flow_dir", flows)
    for extra in (("--temporal_weight", "1"), ("--flow_dir", flows), ("--temporal_init",)):      # sequence flags alone
        with pytest.raises(ValueError):
            RS._video_inputs(_args(*extra))
        with pytest.raises(ValueError):                 # run() refuses before it loads anything
            RS.run(_args(*extra))
    with pytest.raises(ValueError):
        RS._video_inputs(_args(*ok, "--temporal_weight", "-1", content=frames))
    with pytest.raises(ValueError):
        RS._video_inputs(_args(*ok, "--temporal_weight", "nan", content=frames))
    with pytest.raises(ValueError):
        RS._video_inputs(_args(*ok, "--strips", content=frames))
    with pytest.raises(ValueError):
        RS._video_inputs(_args("--video", content=frames))                   # no flows
    with pytest.raises(ValueError):
        RS._video_inputs(_args(*ok, content=os.path.join(frames, "frame_01.png")))      # not a directory
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError):
        RS._video_inputs(_args(*ok, content=frames))
    with pytest.raises(ValueError):
        RS.run(_args(*ok, content=frames))
    monkeypatch.delenv("WORLD_SIZE")
    # a missing backward flow: refused before any frame is optimised
    os.remove(os.path.join(flows, "backward_3_2.flo"))
    with pytest.raises(ValueError, match="backward_3_2"):
        RS._video_inputs(_args(*ok, content=frames))
    with pytest.raises(ValueError):
        RS.run(_args(*ok, "-o", str(tmp_path / "out"), content=frames))
    assert not (tmp_path / "out").exists() or not os.listdir(tmp_path / "out")
    # frames of different sizes
    frames2, flows2 = _sequence(tmp_path / "b")
    Image.new("RGB", (17, 12)).save(os.path.join(frames2, "frame_04.png"))
    T.write_flo(os.path.join(flows2, "backward_4_3.flo"), np.zeros((12, 16, 2), np.float32))
    with pytest.raises(ValueError, match="size"):
        RS._video_inputs(_args("--video", "--flow_dir", flows2, content=frames2))


# ------------------------------------------------------------------ .flo files and the flow resize
def test_read_flo_round_trip_and_bad_files(tmp_path):
    from nn import strotss_utils as SU
    rng = np.random.default_rng(0)
    flow = rng.standard_normal((7, 9, 2)).astype(np.float32) * 5
    T.write_flo(tmp_path / "a.flo", flow)
    got = SU.read_flo(str(tmp_path / "a.flo"))
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 9, 2)
    assert np.array_equal(got.numpy(), flow)
    raw = open(tmp_path / "a.flo", "rb").read()
    open(tmp_path / "magic.flo", "wb").write(np.float32(1.0).tobytes() + raw[4:])
    with pytest.raises(ValueError):
        SU.read_flo(str(tmp_path / "magic.flo"))
    open(tmp_path / "short.flo", "wb").write(raw[:-4])
    with pytest.raises(ValueError):
        SU.read_flo(str(tmp_path / "short.flo"))
    open(tmp_path / "tiny.flo", "wb").write(raw[:6])
    with pytest.raises(ValueError):
        SU.read_flo(str(tmp_path / "tiny.flo"))
    with pytest.raises(FileNotFoundError):
        SU.read_flo(str(tmp_path / "missing.flo"))


def test_resize_flow_scales_the_vectors(monkeypatch):
    from nn import _ops
    from nn import strotss_utils as SU
    flow = torch.from_numpy(np.stack([np.full((6, 8), 4.0), np.full((6, 8), -3.0)], -1).astype(np.float32))
    same = SU.resize_flow(flow, 6, 8)                                   # the same size: the flow itself
    assert torch.equal(same, flow) and same.data_ptr() != flow.data_ptr()
    calls = []

    def fake_resize(x, oh, ow, *a, **k):          # a constant field resizes to the same constant: only the scaling is left
        calls.append((tuple(x.shape), oh, ow))
        return x[:1, :1].expand(oh, ow, 2).contiguous()
    monkeypatch.setattr(_ops, "resize_bilinear", fake_resize)
    monkeypatch.setattr(SU.utils, "device", lambda: torch.device("cpu"))
    got = SU.resize_flow(flow, 3, 12)
    assert calls == [((6, 8, 2), 3, 12)]
    assert tuple(got.shape) == (3, 12, 2)
    assert torch.allclose(got[..., 0], torch.full((3, 12), 4.0 * 12 / 8))       # u * w_new / w_old
    assert torch.allclose(got[..., 1], torch.full((3, 12), -3.0 * 3 / 6))       # v * h_new / h_old
    with pytest.raises(ValueError):
        SU.resize_flow(torch.zeros(6, 8, 3), 3, 4)


# ------------------------------------------------------------------ the float64 restatement on hand cases
def test_integer_translation_warps_exactly_with_an_uncovered_band():
    rng = np.random.default_rng(1)
    h, w, dx, dy = 10, 13, 3, 2
    prev = rng.random((h, w, 3))
    fb = np.broadcast_to(np.float32([-dx, -dy]), (h, w, 2))
    ff = np.broadcast_to(np.float32([dx, dy]), (h, w, 2))
    warped = T.warp64(prev, fb)
    assert np.array_equal(warped[dy:, dx:], prev[:-dy, :-dx])            # exact: whole-pixel samples
    for c in (T.certainty64(fb), T.certainty64(fb, ff)):
        assert np.all(c[dy:, dx:] == 1) and np.all(c[:dy] == 0) and np.all(c[:, :dx] == 0)


def test_flow_out_of_frame_and_inconsistent_flows_have_no_certainty():
    h, w = 8, 8
    out = np.broadcast_to(np.float32([20.0, 0.0]), (h, w, 2))
    assert np.all(T.certainty64(out) == 0)
    zero = np.zeros((h, w, 2), np.float32)
    assert np.all(T.certainty64(zero) == 1) and np.all(T.certainty64(zero, zero) == 1)
    # forward flow that does not bring the pixel back: disoccluded
    assert np.all(T.certainty64(zero, np.broadcast_to(np.float32([2.0, 0.0]), (h, w, 2))) == 0)
    # a step in the backward flow: a motion boundary on both sides of it
    fb = zero.copy()
    fb[:, 4:, 0] = 1.0
    c = T.certainty64(fb)
    assert np.all(c[:, 3:5] == 0) and np.all(c[:, :3] == 1)
    assert np.all(c[:, 5:7] == 1) and np.all(c[:, 7] == 0)          # last column: x + 1 = 8 is out of frame


# ------------------------------------------------------------------ out-of-range and non-finite coordinates
def test_out_of_range_and_non_finite_coordinates_follow_the_rule():
    h, w = 4, 5
    prev = np.arange(h * w * 2, dtype=np.float64).reshape(h, w, 2) + 1.0
    nan, inf = np.nan, np.inf
    for (u, v), (ex, ey) in (((nan, 0), (0, None)), ((0, nan), (None, 0)), ((nan, nan), (0, 0)), ((inf, 0), (w - 1, None)),
                             ((-inf, 0), (0, None)), ((0, inf), (None, h - 1)), ((-inf, inf), (0, h - 1)),
                             ((1e9, -1e9), (w - 1, 0)), ((-7.5, 0), (0, None)), ((0, 9.25), (None, h - 1)),
                             ((-0.5, 0), (None, None))):
        fb = np.zeros((h, w, 2), np.float32)
        fb[2, 2] = (u, v)
        warped, cert = T.warp64(prev, fb), T.certainty64(fb)
        assert np.isfinite(warped).all()
        if (u, v) == (-0.5, 0):                          # an ordinary sample: halfway between two pixels, in frame
            assert np.array_equal(warped[2, 2], 0.5 * (prev[2, 1] + prev[2, 2])) and cert[2, 2] == 1
            continue
        x, y = (2 if ex is None else ex), (2 if ey is None else ey)
        assert np.array_equal(warped[2, 2], prev[y, x]), (u, v)          # the edge pixel of the axis, exactly
        assert cert[2, 2] == 0, (u, v)
        untouched = np.ones((h, w), bool)
        untouched[2, 2] = False
        assert np.array_equal(warped[untouched], prev[untouched])
        # the four neighbours' motion-boundary tests read the planted vector: a NaN difference is not `>` the threshold and
        # removes nothing; an infinite or huge one removes the neighbours along its axis
        near = [(1, 2), (3, 2), (2, 1), (2, 3)]
        kept = 1 if np.isnan(u) or np.isnan(v) else 0
        for p in near:
            assert cert[p] == kept, ((u, v), p)
        far = untouched.copy()
        for p in near:
            far[p] = False
        assert (cert[far] == 1).all()
    # a forward flow is sampled by the same rule; a NaN or infinite sample of it fails no test (NaN > x and inf > inf are false)
    zero = np.zeros((h, w, 2), np.float32)
    ff = zero.copy()
    ff[1, 1] = (nan, 0)
    ff[2, 3] = (inf, inf)
    assert (T.certainty64(zero, ff) == 1).all()
    ff[3, 4] = (2.0, 0)                                  # and an ordinary wrong one does (no tap of (3, 4) is non-finite; at
    assert T.certainty64(zero, ff)[3, 4] == 0            # (0, 0) the zero-weight tap (1, 1) would make the sample NaN)
    # a sample out of range never consults the forward flow: certainty 0 whatever it holds there
    out = np.broadcast_to(np.float32([w + 3.0, 0.0]), (h, w, 2))
    assert (T.certainty64(out, ff) == 0).all() and np.array_equal(T.warp64(prev, out), np.repeat(prev[:, -1:], w, axis=1))


def test_samples_on_the_last_row_and_column_are_in_frame_and_the_next_float_is_not():
    h, w = 6, 9
    prev = np.random.default_rng(0).random((h, w, 3)).astype(np.float32)
    one, beyond = np.float32(1), np.nextafter(np.float32(1), np.float32(np.inf))
    for axis in (0, 1):
        on = np.zeros((h, w, 2), np.float32)
        on[..., axis] = one
        past = np.zeros((h, w, 2), np.float32)
        past[..., axis] = beyond
        c_on, c_past = T.certainty64(on), T.certainty64(past)
        assert (c_on[:h - 1, :] == 1).all() if axis else (c_on[:, :w - 1] == 1).all()
        if axis == 0:
            assert (c_on[:, w - 2] == 1).all() and (c_on[:, w - 1] == 0).all()        # x + u == w - 1: in frame
            assert (c_past[:, w - 2] == 0).all() and (c_past[:, :w - 2] == 1).all()   # the next float: out
            assert np.array_equal(T.warp64(prev, on)[:, :w - 1], prev[:, 1:])          # and the value is exact
        else:
            assert (c_on[h - 2] == 1).all() and (c_on[h - 1] == 0).all()
            assert (c_past[h - 2] == 0).all() and (c_past[:h - 2] == 1).all()
            assert np.array_equal(T.warp64(prev, on)[:h - 1], prev[1:])


def test_slack_option_measures_the_distance_to_the_thresholds():
    h, w = 5, 6
    zero = np.zeros((h, w, 2), np.float32)
    c, s = T.certainty64(zero, slack=True)
    assert (c == 1).all() and (s == 1).all()             # 0 against 0.002: relative slack 1
    fb = zero.copy()
    fb[:, 3:, 0] = np.float32(0.0895)                    # a step whose central difference squared is 0.00200256: just above 0.002
    c, s = T.certainty64(fb, slack=True)
    assert c[2, 2] == 0 and 0 < s[2, 2] < 2e-3
    assert np.array_equal(c, T.certainty64(fb))
    out = np.broadcast_to(np.float32([20.0, 0.0]), (h, w, 2))
    assert np.isinf(T.certainty64(out, zero, slack=True)[1]).all()       # out of frame: no threshold test is evaluated


@pytest.mark.parametrize("hw", T.WARP_SHAPES, ids=[f"{h}x{w}" for h, w in T.WARP_SHAPES])
def test_warp_cases_meet_their_conditions(hw):
    h, w = hw
    cases = T.warp_cases(h, w)
    names = [n for n, _, _ in cases]
    assert len(set(names)) == len(names)
    assert {"smooth", "planted", "far", "whole(0,0)", "whole(1,0)", "half(1.5,-1.5)", "half(-1.5,0)"} <= set(names)
    assert sum(n.startswith("half") for n in names) == 8 and sum(n.startswith("beyond") for n in names) == 3
    prevs = {c: T.warp_prev(h, w, c) for c in T.WARP_CHANNELS}
    worst = np.inf
    for name, fb, ff in cases:
        assert fb.dtype == np.float32 and ff.dtype == np.float32 and fb.shape == ff.shape == (h, w, 2)
        for f in (None, ff):
            cert, slack = T.certainty64(fb, f, slack=True)
            assert set(np.unique(cert)) <= {0.0, 1.0}
            assert slack.min() > T.SLACK_MARGIN, (name, f is not None, slack.min())
            worst = min(worst, float(slack.min()))
        for c, prev in prevs.items():
            assert np.isfinite(T.warp64(prev, fb)).all(), (name, c)
    print(f"{h} x {w}: {len(cases)} cases, smallest slack of an evaluated threshold test {worst:.3e} (margin {T.SLACK_MARGIN:g})")
    by = {n: (fb, ff) for n, fb, ff in cases}
    assert (T.certainty64(*by["whole(0,0)"]) == 1).all()
    assert (T.certainty64(*by["far"]) == 0).all()
    assert np.array_equal(T.warp64(prevs[3], by["far"][0]), np.broadcast_to(prevs[3][0, w - 1].astype(np.float64), (h, w, 3)))
    # x + u == w - 1 is in frame and exact; the next float32 is out
    on, past = T.certainty64(by["whole(1,0)"][0]), T.certainty64(by["beyond(1,0)"][0])
    if w >= 2:
        assert (on[:, w - 2] == 1).all() and (past[:, w - 2] == 0).all()
        assert np.array_equal(T.warp64(prevs[4], by["whole(1,0)"][0])[:, w - 2], prevs[4][:, w - 1])
    assert (on[:, w - 1] == 0).all()
    on, past = T.certainty64(by["whole(0,1)"][0]), T.certainty64(by["beyond(0,1)"][0])
    if h >= 2:
        assert (on[h - 2] == 1).all() and (past[h - 2] == 0).all()
    # the half-pixel shifts leave a band off each side and corner
    for (dx, dy) in T.HALF_SHIFTS:
        cert = T.certainty64(by[f"half({dx:g},{dy:g})"][0])
        assert cert.sum() == max(w - 2 * (dx != 0), 0) * max(h - 2 * (dy != 0), 0)
    fb = by["planted"][0]
    planted = ~np.isfinite(fb).all(-1) | (np.abs(fb) > 1e8).any(-1)
    assert planted.sum() == min(len(T.PLANTED), h * w) and (T.certainty64(fb)[planted] == 0).all()
    if h * w > 1000:                                     # ordinary pixels among them, both kinds of certainty
        assert 0.5 * h * w < T.certainty64(*by["planted"]).sum() < h * w - planted.sum()
        assert 0.2 * h * w < T.certainty64(*by["smooth"]).sum() < T.certainty64(by["smooth"][0]).sum()


@pytest.mark.parametrize("with_forward", [False, True])
@pytest.mark.parametrize("hw", [(40, 56), (33, 71)])
def test_the_random_cases_of_the_device_test_keep_the_margin(with_forward, hw):
    _, fb, ff = T.random_warp_case(*hw, with_forward)
    got = T.min_slack(fb, ff)
    print(f"{hw}, forward flow {with_forward}: smallest slack {got:.3e}")
    assert got > T.SLACK_MARGIN


def test_temporal_loss_restatement():
    rng = np.random.default_rng(2)
    h, w = 5, 7
    x, tgt, c = rng.random((h, w, 3)), rng.random((h, w, 3)), (rng.random((h, w)) > 0.3).astype(np.float64)
    loss, grad = T.temporal_loss64(x, tgt, c)
    assert abs(loss - sum(c[i, j] * ((x[i, j] - tgt[i, j]) ** 2).sum() for i in range(h) for j in range(w)) / (3 * h * w)) < 1e-15
    eps = 1e-6
    x2 = x.copy()
    x2[1, 2, 0] += eps
    assert abs((T.temporal_loss64(x2, tgt, c)[0] - loss) / eps - grad[1, 2, 0]) < 1e-6
    assert T.temporal_loss64(x, tgt, np.zeros((h, w)))[0] == 0.0 and not grad[c == 0].any()


# ------------------------------------------------------------------ refused C calls
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_library_exports_the_temporal_entries(lib):
    for s in ("strotss_flow_warp", "strotss_temporal_fwd_bwd", "strotss_temporal_workspace_bytes"):
        assert hasattr(lib, s)
    assert lib.strotss_abi_version() == 8
    assert lib.strotss_temporal_workspace_bytes(0, 4) == 0 and lib.strotss_temporal_workspace_bytes(4, -1) == 0
    assert lib.strotss_temporal_workspace_bytes(64, 64) >= 16 + 4


def test_flow_warp_refuses_before_launching(lib):
    def call(prev=P, h=8, w=8, c=3, fb=P, ff=None, out=P, cert=P):
        return lib.strotss_flow_warp(prev, h, w, c, fb, ff, out, cert, None)
    assert call(prev=None) == EINVAL and call(fb=None) == EINVAL and call(out=None) == EINVAL and call(cert=None) == EINVAL
    assert call(h=0) == EINVAL and call(w=-1) == EINVAL and call(c=0) == EINVAL


def test_temporal_fwd_bwd_refuses_before_launching(lib):
    f = C.c_float(1.0)

    def call(img=P, tgt=P, cert=P, h=8, w=8, g=P, loss=P, ws=P):
        return lib.strotss_temporal_fwd_bwd(img, tgt, cert, h, w, f, g, loss, ws, None)
    assert call(img=None) == EINVAL and call(tgt=None) == EINVAL and call(cert=None) == EINVAL
    assert call(g=None) == EINVAL and call(loss=None) == EINVAL and call(ws=None) == EINVAL
    assert call(h=0) == EINVAL and call(w=-2) == EINVAL
    assert call(g=ODD) == EALIGN and call(img=ODD) == EALIGN and call(tgt=ODD) == EALIGN and call(cert=ODD) == EALIGN
    assert call(ws=ODD) == EALIGN
