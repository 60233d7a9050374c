"""Content-weight map without a GPU: the --content_weight_map command line and its refusals, the checks of the weight-map
helper, the float64 restatement of the weighted content loss (all ones = self_similarity; symmetric in its two row sets),
the map loader, and the status codes of refused weighted C calls (checked before anything launches)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

EINVAL, EALIGN, ERANGE = -1, -2, -3
P = C.c_void_p(0x10000)          # "some buffer": non-null, never touched
WS = 1 << 30


def _args(*extra):
    import run_strotss as RS
    return RS.build_parser().parse_args(["c.jpg", "s.jpg", *extra])


def test_content_weight_map_flag_parses():
    assert _args("--content_weight_map", "m.png").content_weight_map == "m.png"
    assert _args().content_weight_map is None
    a = _args("--content_weight_map", "m.png", "--style_mix", "a.jpg", "--content_mask", "cm.jpg", "--style_mask", "sm.jpg")
    assert a.content_weight_map == "m.png" and a.style_mix == ["a.jpg"]


def test_content_weight_input_wiring_and_refusals(monkeypatch):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    assert RS._content_weight_input(_args()) is None
    assert RS._content_weight_input(_args("--content_weight_map", "m.png")) == "m.png"
    # combines with masks and style blends
    assert RS._content_weight_input(_args("--content_weight_map", "m.png", "--style_mix", "a.jpg", "--content_mask", "c",
                                          "--style_mask", "s")) == "m.png"
    with pytest.raises(ValueError):
        RS._content_weight_input(_args("--content_weight_map", "m.png", "--strips"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError):
        RS._content_weight_input(_args("--content_weight_map", "m.png"))
    with pytest.raises(ValueError):                      # run() refuses before it loads anything
        RS.run(_args("--content_weight_map", "m.png"))
    assert RS._content_weight_input(_args()) is None     # no map: a multi-process run is not this flag's business


@pytest.mark.parametrize("bad", [
    -np.ones((8, 8), dtype=np.float32),                                  # negative
    np.array([[0.5, np.nan], [0.5, 0.5]], dtype=np.float32),             # NaN
    np.array([[0.5, np.inf], [0.5, 0.5]], dtype=np.float32),             # infinite
    np.ones((2, 8, 8), dtype=np.float32),                                # wrong shape
    np.ones((8,), dtype=np.float32),
])
def test_content_weight_at_scale_refuses(bad):
    from nn import strotss_utils as SU
    with pytest.raises(ValueError):
        SU.content_weight_at_scale(torch.from_numpy(bad), 4, 4)


def test_check_content_weight_shapes_and_values():
    from nn import strotss_utils as SU
    m = torch.rand(6, 5) * 2.0                                           # values above 1 pass the Python API
    out = SU.check_content_weight(m, 6, 5)
    assert tuple(out.shape) == (1, 6, 5, 1) and out.dtype == torch.float32 and torch.equal(out[0, ..., 0], m)
    assert torch.equal(SU.check_content_weight(out, 6, 5), out)
    for bad in (torch.rand(5, 6), torch.rand(1, 6, 5, 2), -m, m.masked_fill(m > 1.5, float("nan"))):
        with pytest.raises(ValueError):
            SU.check_content_weight(bad, 6, 5)


def test_load_content_weight_map(tmp_path):
    from PIL import Image
    from nn import strotss_utils as SU
    rgb = np.zeros((6, 9, 3), dtype=np.uint8)
    rgb[:, :3] = 255
    rgb[:, 3:6] = (255, 0, 0)
    Image.fromarray(rgb).save(tmp_path / "m.png")
    m = SU.load_content_weight_map(str(tmp_path / "m.png"))
    grey = np.asarray(Image.fromarray(rgb).convert("L"), dtype=np.float32)
    assert tuple(m.shape) == (6, 9) and m.dtype == torch.float32
    assert torch.equal(m, torch.from_numpy(grey / np.float32(255)))
    assert bool((m[:, :3] == 1.0).all()) and bool((m[:, 6:] == 0.0).all())       # white is exactly 1
    with pytest.raises(FileNotFoundError):
        SU.load_content_weight_map(str(tmp_path / "missing.png"))


# ------------------------------------------------------------------ float64 restatement of the weighted content loss
def weighted_selfsim64(x, y, c):
    from oracle import strotss_oracle as O

    def cols(z):
        dz = O.cosine_distance(z, z)
        return dz / torch.clamp(dz.sum(dim=0), min=1e-12)
    return (c[None, :] * (cols(x) - cols(y)).abs()).sum() / x.shape[0]


def test_weighted_restatement_all_ones_is_self_similarity_and_symmetric():
    from nn import strotss_utils as SU
    from oracle import strotss_oracle as O
    g = torch.Generator().manual_seed(0)
    x, y = torch.rand(40, 7, generator=g, dtype=torch.float64), torch.rand(40, 7, generator=g, dtype=torch.float64)
    ones = SU.check_content_weight(torch.ones(5, 8), 5, 8).reshape(-1).double()       # an all-white 5 x 8 map's samples
    assert abs(float(weighted_selfsim64(x, y, ones) - O.self_similarity(x, y))) < 1e-12
    c = torch.rand(40, generator=g, dtype=torch.float64)
    c[::5] = 0.0
    c = SU.check_content_weight(c.reshape(5, 8), 5, 8).reshape(-1).double()
    a, b = weighted_selfsim64(x, y, c), weighted_selfsim64(y, x, c)
    assert abs(float(a - b)) < 1e-14
    assert float(weighted_selfsim64(x, y, torch.zeros(40, dtype=torch.float64))) == 0.0
    # linear in the map: the sum of the loss over two maps is the loss of their sum
    c2 = torch.rand(40, generator=g, dtype=torch.float64)
    assert abs(float(weighted_selfsim64(x, y, c) + weighted_selfsim64(x, y, c2) - weighted_selfsim64(x, y, c + c2))) < 1e-12


def test_weighted_self_similarity_refuses_bad_weights():
    from nn.losses import weighted_self_similarity
    x, y = torch.rand(10, 5), torch.rand(10, 5)
    for bad in (torch.ones(9), -torch.ones(10), torch.full((10,), float("nan"))):
        with pytest.raises(ValueError):
            weighted_self_similarity(x, y, bad)
    with pytest.raises(ValueError):
        weighted_self_similarity(x, torch.rand(11, 5), torch.ones(10))


# ------------------------------------------------------------------ refused C calls
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_selfsim_weighted_entry_refuses_before_launching(lib):
    f = C.c_float(1.0)

    def call(pred=P, content=P, n=1024, d=2179, ld=2208, gpred=P, loss=P, ws=P):
        return lib.strotss_selfsim_weighted_fwd_bwd(pred, content, P, n, d, ld, f, gpred, loss, ws, WS, None)
    assert call(pred=None) == EINVAL and call(content=None) == EINVAL
    assert call(gpred=None) == EINVAL and call(loss=None) == EINVAL and call(ws=None) == EINVAL
    assert call(n=0) == EINVAL and call(n=-3) == EINVAL and call(d=0) == EINVAL
    assert call(ld=2176) == EINVAL                      # ld < d
    assert call(ld=2180) == EALIGN                      # ld % 32 != 0
    assert lib.strotss_selfsim_weighted_fwd_bwd(P, P, P, 1024, 2179, 2208, f, P, P, P, 16, None) == EINVAL   # workspace short


def _set(k=1, ns=1024):
    from nn import _hip
    s = _hip.StyleSetT()
    s.n_styles = k
    for i in range(min(k, _hip.MAX_STYLES)):
        s.feats[i] = s.inv_norm[i] = s.panels[i] = s.mean[i] = s.cov[i] = P.value
        s.ns[i] = ns
        s.weight[i] = 1.0
    return s


@pytest.mark.parametrize("k", [1, 2])
def test_step_losses_cw_entry_refuses_before_launching(lib, k):
    f = C.c_float(1.0)

    def call(pred=P, content=P, n=1024, d=2179, ld=2208, styles=True, s=None, gpred=P):
        st = C.byref(s if s is not None else _set(k)) if styles else None
        return lib.strotss_step_losses_cw_fwd_bwd(pred, content, n, d, ld, P, st, f, f, f, f, gpred, P, P, P, P, P, WS, None)
    assert call(pred=None) == EINVAL and call(content=None) == EINVAL and call(gpred=None) == EINVAL
    assert call(styles=False) == EINVAL
    assert call(n=0) == EINVAL and call(n=-1) == EINVAL
    assert call(ld=2180) == EALIGN
    assert call(ld=2176) == EINVAL
    assert call(s=_set(0)) == ERANGE and call(s=_set(5)) == ERANGE
    assert call(s=_set(k, ns=4096)) == ERANGE


def test_gather2_cw_entry_refuses_before_launching(lib):
    from nn import _hip
    maps = _hip.MapsT()
    maps.n_maps, maps.h[0], maps.w[0], maps.c[0], maps.map[0] = 1, 8, 8, 3, P.value
    wmap = _hip.MapsT()
    wmap.n_maps, wmap.h[0], wmap.w[0], wmap.c[0], wmap.map[0] = 1, 8, 8, 1, P.value

    def call(mw=wmap, idx=P, n=16, out=P, ld=32, wout=P, wrows=32):
        return lib.strotss_hypercol_gather2_cw(C.byref(maps), C.byref(maps), C.byref(mw) if mw is not None else None, idx, n, 1,
                                               out, out, ld, None, 0, wout, wrows, None)
    assert call(mw=None) == EINVAL and call(idx=None) == EINVAL and call(out=None) == EINVAL and call(wout=None) == EINVAL
    assert call(n=0) == EINVAL
    assert call(wrows=15) == EINVAL                      # fewer weight rows than samples
    assert call(mw=maps) == EINVAL                       # the weight map has one channel
    two = _hip.MapsT.from_buffer_copy(wmap)
    two.n_maps, two.h[1], two.w[1], two.c[1], two.map[1] = 2, 8, 8, 1, P.value
    assert call(mw=two) == EINVAL                        # and is one map
    assert call(ld=2) == EINVAL                          # ld < channels of the feature maps
