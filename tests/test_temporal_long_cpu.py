"""Long-term temporal consistency without a GPU: the --temporal_frames command line and its refusals
(all raised before run() loads anything), the exported entries and their refused calls (checked before anything launches),
and the float64 restatement of the combined certainties and of L_t = sum_j L_j on hand-computed cases."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _temporal_long_ref as TL  # noqa: E402
import _temporal_ref as T  # noqa: E402

EINVAL, EALIGN = -1, -2
P = 0x10000          # "some buffer": non-null, 16-byte aligned, never touched
ODD = 0x10004        # non-null, not 16-byte aligned


def _args(*extra, content="c.jpg"):
    import run_strotss as RS
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


def _sequence(tmp_path, n=4, offsets=(1, 2)):
    frames, flows = tmp_path / "frames", tmp_path / "flows"
    TL.occluder_sequence(str(frames), str(flows), n_frames=n, h=24, w=40, size=6, vx=5, y0=8, offsets=offsets)
    return str(frames), str(flows)


# ------------------------------------------------------------------ command line
def test_temporal_frames_flag_parses():
    import run_strotss as RS
    a = _args("--video", "--flow_dir", "f", "--temporal_frames", "1", "10", "20", "40")
    assert a.temporal_frames == [1, 10, 20, 40]
    assert RS._temporal_frames(a) == (1, 10, 20, 40)
    a = _args()
    assert a.temporal_frames is None and RS._temporal_frames(a) == (1,)          # the default: the short-term term
    assert RS._temporal_frames(_args("--video", "--temporal_frames", "20", "1", "10")) == (1, 10, 20)    # ascending
    assert RS._temporal_frames(_args("--video", "--temporal_frames", "3")) == (3,)
    assert "--temporal_frames" in RS.__doc__ and "--temporal_frames" in RS.build_parser().format_help()


def test_temporal_frames_wiring(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames, flows = _sequence(tmp_path)
    got, lam = RS._video_inputs(_args("--video", "--flow_dir", flows, "--temporal_frames", "1", "2", content=frames))
    assert len(got) == 4 and lam == RS.DEFAULT_TEMPORAL_WEIGHT
    # offsets larger than the sequence apply to no frame: nothing to read for them
    assert RS._video_inputs(_args("--video", "--flow_dir", flows, "--temporal_frames", "1", "2", "9", content=frames))


def test_temporal_frames_refusals(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames, flows = _sequence(tmp_path)
    out = tmp_path / "out"
    ok = ("--video", "--flow_dir", flows, "-o", str(out))
    with pytest.raises(ValueError, match="needs --video"):              # the flag alone
        RS._video_inputs(_args("--temporal_frames", "1", "2"))
    with pytest.raises(ValueError, match="needs --video"):
        RS.run(_args("--temporal_frames", "1", "2"))
    for bad in (("0",), ("-1",), ("1", "0"), ("1", "2", "1"), ("2", "2"), ("1", "2", "3", "4", "5")):
        with pytest.raises(ValueError, match="--temporal_frames"):
            RS._video_inputs(_args(*ok, "--temporal_frames", *bad, content=frames))
        with pytest.raises(ValueError, match="--temporal_frames"):     # run() refuses before it loads anything
            RS.run(_args(*ok, "--temporal_frames", *bad, content=frames))
    assert not out.exists()
    # a missing long-term backward flow of an applicable (t, j): refused, the file named
    os.remove(os.path.join(flows, "backward_4_2.flo"))
    assert RS._video_inputs(_args(*ok, content=frames))                 # J = {1} does not need it
    with pytest.raises(ValueError, match="backward_4_2.flo"):
        RS._video_inputs(_args(*ok, "--temporal_frames", "1", "2", content=frames))
    with pytest.raises(ValueError, match="backward_4_2.flo"):
        RS.run(_args(*ok, "--temporal_frames", "1", "2", content=frames))
    assert not out.exists()
    with pytest.raises(ValueError, match="backward_4_2.flo"):           # an offset alone, without 1
        RS._video_inputs(_args(*ok, "--temporal_frames", "2", content=frames))


@pytest.mark.parametrize("track", (False, True), ids=("plain", "tracked"))
@pytest.mark.parametrize("offsets", ((1, 2), (1,)))
def test_each_frame_offset_pair_is_computed_once(tmp_path, monkeypatch, offsets, track):
    """run_video on four frames with everything around the pairs stubbed: one _flow_warp_for_frame call per (t, j) with
    t - j >= 1, its entry handed to the tracking and to the temporal list as the same objects, one pair with its raw
    certainty, two combined by one temporal_long_certainty call with the planes nearest first."""
    import torch
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    names = [f"f{t}.jpg" for t in (1, 2, 3, 4)]
    results, made, tracked, stylised, combined = {}, {}, [], [], []

    def flow_warp(args, t, previous, j=1, frames=None):
        assert (t, j) not in made, f"pair {(t, j)} computed twice"
        assert previous is results[t - j]                              # the optimiser's own result of frame t-j
        made[(t, j)] = (object(), object(), torch.full((2, 3), float(10 * t + j)))
        return made[(t, j)]

    def long_certainty(stack):
        combined.append(stack.clone())
        return stack + 0.5

    def stylise(job, vgg, frame, dev, **kw):
        t = names.index(frame) + 1
        stylised.append((t, kw["temporal"], kw["masks"]))
        results[t] = torch.full((1, 2, 3, 3), float(t))
        return results[t]

    def tracked_masks(job, vgg, tracking, t, frame, nearest):
        tracked.append((t, job.offsets[0], nearest))
        return [None], [None]

    def video_inputs(args, found):                                     # no frame files: the names, the offsets as parsed
        found.update(match_radius=0, robust=None, offsets=RS._temporal_frames(args))
        return names, 1.0

    monkeypatch.setattr(RS, "_video_inputs", video_inputs)
    monkeypatch.setattr(RS, "VGG", lambda **kw: None)
    monkeypatch.setattr(RS, "_flow_warp_for_frame", flow_warp)
    monkeypatch.setattr(RS.strotss_engine._ops, "temporal_long_certainty", long_certainty)
    monkeypatch.setattr(RS, "_stylise", stylise)
    monkeypatch.setattr(RS, "_tracked_masks", tracked_masks)
    monkeypatch.setattr(RS, "_written", lambda stylized, post, guides: stylized)
    monkeypatch.setattr(RS.utils, "write_image", lambda image, path: None)
    extra = ("--auto_masks", "3", "--track_masks") if track else ()
    outs = RS.run_video(_args("--video", "--flow_dir", "f", "--temporal_frames", *map(str, offsets), *extra,
                              "-o", str(tmp_path / "out"), content="frames"))
    assert len(outs) == 4
    assert sorted(made) == [(t, j) for t in (1, 2, 3, 4) for j in offsets if t - j >= 1]
    assert [t for t, _, _ in stylised] == [1, 2, 3, 4]
    assert [(t, j) for t, j, _ in tracked] == ([(t, offsets[0]) for t in (1, 2, 3, 4)] if track else [])
    for t, j, nearest in tracked:                                      # the tracking's pair is the map's entry itself
        assert nearest is made.get((t, j))
    n_combined = 0
    for t, temporal, masks in stylised:
        js = [j for j in offsets if t - j >= 1]                        # nearest frame first
        assert len(temporal) == len(js) and (masks is not None) == track
        assert all(pair[0] is made[(t, j)][1] for pair, j in zip(temporal, js))
        if len(js) == 1:                                               # one pair: the raw certainty, untouched
            assert temporal[0][1] is made[(t, js[0])][2]
        elif js:
            raw = torch.stack([made[(t, j)][2] for j in js])
            assert torch.equal(combined[n_combined], raw)
            assert all(torch.equal(pair[1], raw[k] + 0.5) for k, pair in enumerate(temporal))
            n_combined += 1
    assert len(combined) == n_combined == sum(1 for t in (1, 2, 3, 4) if sum(t - j >= 1 for j in offsets) >= 2)


def test_the_occluder_sequence_is_what_it_says(tmp_path):
    from PIL import Image
    frames, flows = tmp_path / "f", tmp_path / "fl"
    paths, occluder = TL.occluder_sequence(str(frames), str(flows), n_frames=4)
    imgs = [np.asarray(Image.open(p), dtype=np.float64) / 255 for p in paths]
    for t in (2, 3, 4):
        for j in (1, 2):
            if t - j < 1:
                continue
            from nn import strotss_utils as SU
            fb = SU.read_flo(str(flows / f"backward_{t}_{t - j}.flo")).numpy()
            rel = np.asarray(Image.open(flows / f"reliable_{t}_{t - j}.pgm"), dtype=np.float64) / 255
            # where the pgm is certain, frame t-j warped along the exact flow IS frame t
            warped = T.warp64(imgs[t - j - 1], fb)
            assert np.abs(warped - imgs[t - 1])[rel == 1].max() < 1e-12
            assert (rel == 0).sum() == (occluder(t - j) & ~occluder(t)).sum() > 0
    # pixels visible in t-2 and t but covered in t-1: what the long-term term is for
    for t in (3, 4):
        assert (occluder(t - 1) & ~occluder(t) & ~occluder(t - 2)).sum() > 0


# ------------------------------------------------------------------ the float64 restatement on hand cases
def test_combined_certainty_hand_case():
    raw = np.array([[[1.0, 0.0, 0.25, 0.0]],          # nearest frame
                    [[1.0, 1.0, 1.0, 0.5]],
                    [[0.5, 1.0, 0.5, 1.0]]])
    want = np.array([[[1.0, 0.0, 0.25, 0.0]],
                     [[0.0, 1.0, 0.75, 0.5]],
                     [[0.0, 0.0, 0.0, 0.5]]])
    assert np.array_equal(TL.long_certainty64(raw), want)
    assert np.array_equal(TL.long_certainty32(raw), want.astype(np.float32))
    rng = np.random.default_rng(0)
    for count in (1, 2, 3, 4):
        st = rng.random((count, 9, 11)).astype(np.float32)
        st[rng.random(st.shape) < 0.3] = 0.0
        c32, c64 = TL.long_certainty32(st), TL.long_certainty64(st)
        assert np.array_equal(c32[0], st[0]) and (c32 >= 0).all()
        assert np.abs(c32 - c64).max() < 1e-6
        # binary certainties: each pixel pulls toward its nearest covering frame only
        b = (st > 0.5).astype(np.float32)
        cb = TL.long_certainty32(b)
        assert np.array_equal(cb, TL.long_certainty64(b).astype(np.float32))
        assert cb.sum(axis=0).max() <= 1 and np.array_equal(cb.sum(axis=0), b.max(axis=0))


def test_multi_term_loss_hand_case():
    h, w = 1, 2
    x = np.zeros((h, w, 3))
    t1 = np.ones((h, w, 3))
    t2 = np.full((h, w, 3), 2.0)
    c1 = np.array([[1.0, 0.0]])
    c2 = np.array([[1.0, 1.0]])
    raw = np.stack([c1, c2])
    c = TL.long_certainty64(raw)                          # [[1, 0]], [[0, 1]]
    losses, grad = TL.multi_loss64(x, [t1, t2], list(c), [3.0, 5.0])
    # L_1 = (1/6) * 1 * 3 * 1^2, L_2 = (1/6) * 1 * 3 * 2^2 (pixel 1 only)
    assert losses == [0.5, 2.0]
    assert np.allclose(grad[0, 0], -1.0, rtol=1e-14, atol=0)              # 3 * 2 * (0 - 1) / 6
    assert np.allclose(grad[0, 1], -10.0 / 3, rtol=1e-14, atol=0)         # 5 * 2 * (0 - 2) / 6
    eps = 1e-6
    x2 = x.copy()
    x2[0, 1, 2] += eps
    l2, _ = TL.multi_loss64(x2, [t1, t2], list(c), [3.0, 5.0])
    assert abs((3.0 * (l2[0] - losses[0]) + 5.0 * (l2[1] - losses[1])) / eps - grad[0, 1, 2]) < 1e-5
    # one target: the single-term restatement itself
    l, g = T.temporal_loss64(x, t1, c1)
    lm, gm = TL.multi_loss64(x, [t1], [c1], [1.0])
    assert lm == [l] and np.array_equal(gm, g)


# ------------------------------------------------------------------ the C entries: exported, refused before launching
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_library_exports_the_long_term_entries(lib):
    from nn import _hip
    for s in ("strotss_temporal_long_certainty", "strotss_temporal_multi_fwd_bwd", "strotss_temporal_multi_workspace_bytes"):
        assert hasattr(lib, s) and s in _hip.SIGNATURES
    assert lib.strotss_abi_version() == 8 and _hip.MAX_TEMPORAL == 4
    ws = lib.strotss_temporal_multi_workspace_bytes
    assert ws(0, 4, 2) == 0 and ws(4, -1, 2) == 0 and ws(64, 64, 0) == 0 and ws(64, 64, 5) == 0
    assert ws(64, 64, 1) == lib.strotss_temporal_workspace_bytes(64, 64)          # count 1: the single-term layout
    assert ws(64, 64, 4) == 16 + 4 * 4 * 4 and ws(33, 33, 3) == 16 + 4 * 3 * 2


def test_long_certainty_refuses_before_launching(lib):
    def call(raw=P, count=2, h=8, w=8, out=P):
        return lib.strotss_temporal_long_certainty(raw, count, h, w, out, None)
    assert call(raw=None) == EINVAL and call(out=None) == EINVAL
    assert call(count=0) == EINVAL and call(count=5) == EINVAL and call(count=-1) == EINVAL
    assert call(h=0) == EINVAL and call(w=-3) == EINVAL
    assert call(h=40000, w=20000) == EINVAL                # 3 h w > INT_MAX
    assert call(raw=ODD) == EALIGN and call(out=ODD) == EALIGN


def test_multi_fwd_bwd_refuses_before_launching(lib):
    from nn import _hip

    def set_(count=3, tgt=P, cert=P, bad=None):
        s = _hip.TemporalSetT()
        s.count = count
        for j in range(_hip.MAX_TEMPORAL):
            s.target[j], s.certainty[j], s.gscale[j] = tgt, cert, 1.0
        if bad is not None:
            field, j, val = bad
            getattr(s, field)[j] = val
        return s

    # every call below has exactly one bad argument: none may reach a launch (the pointers are fake)
    def call(img=P, s=None, h=8, w=8, g=P, loss=P, ws=P):
        return lib.strotss_temporal_multi_fwd_bwd(img, C.byref(s), h, w, g, loss, ws, None)

    def ok(**kw):
        return dict(s=set_(), **kw)
    assert lib.strotss_temporal_multi_fwd_bwd(P, None, 8, 8, P, P, P, None) == EINVAL            # no set
    assert call(**ok(img=None)) == EINVAL and call(**ok(g=None)) == EINVAL
    assert call(**ok(loss=None)) == EINVAL and call(**ok(ws=None)) == EINVAL
    assert call(**ok(h=0)) == EINVAL and call(**ok(w=-2)) == EINVAL
    assert call(**ok(h=40000, w=20000)) == EINVAL
    for count in (0, 5, -1):
        assert call(s=set_(count)) == EINVAL
    assert call(s=set_(bad=("target", 2, None))) == EINVAL and call(s=set_(bad=("certainty", 0, None))) == EINVAL
    assert call(**ok(img=ODD)) == EALIGN and call(**ok(g=ODD)) == EALIGN and call(**ok(ws=ODD)) == EALIGN
    assert call(s=set_(bad=("target", 1, ODD))) == EALIGN and call(s=set_(bad=("certainty", 2, ODD))) == EALIGN
