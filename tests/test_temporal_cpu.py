"""Temporal consistency of frame sequences without a GPU: the --video / --flow_dir / --temporal_weight / --temporal_init
command line and its refusals, the .flo reader, the flow resize's vector scaling, the float64 restatement of the warp, the
certainty and L_t on hand cases, and the status codes of refused strotss_flow_warp / strotss_temporal_fwd_bwd calls (checked
before anything launches)."""
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
