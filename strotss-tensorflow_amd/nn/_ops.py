"""Tensor-level wrappers over the C ABI (one Python function per entry point of
include/strotss_hip.h).  Tensors are torch HIP tensors used purely as device memory."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _hip
from ._hip import check, ptr, require, stream_ptr

IMAGENET_MEAN = (0.485, 0.456, 0.406)      # reference nn/model.py:34
IMAGENET_STD = (0.229, 0.224, 0.225)       # reference nn/model.py:35
_MEAN3 = (C.c_float * 3)(*IMAGENET_MEAN)
_STD3 = (C.c_float * 3)(*IMAGENET_STD)


def pad32(v: int) -> int:
    return (v + 31) // 32 * 32


def canonical_device(device) -> torch.device:
    """torch.device with an explicit index ("cuda" -> "cuda:<current>"), comparable with Tensor.device."""
    d = torch.device(device)
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def hwc(t: torch.Tensor) -> Tuple[int, int, int]:
    return int(t.shape[-3]), int(t.shape[-2]), int(t.shape[-1])


# ------------------------------------------------------------------ images
def resize_bilinear(x: torch.Tensor, oh: int, ow: int, alpha: float = 1.0,
                    add: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    require(x, "resize input")
    ih, iw, c = hwc(x)
    shape = (*x.shape[:-3], oh, ow, c)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    if add is not None:
        require(add, "resize addend")
        assert add.numel() == out.numel()
    check(_hip.lib().strotss_resize_bilinear(ptr(x), ih, iw, c, ptr(out), oh, ow, alpha, ptr(add),
                                             stream_ptr()), "resize_bilinear")
    return out


def fold_pyramid(variables: Sequence[torch.Tensor], out: torch.Tensor) -> Optional[torch.Tensor]:
    """out = fold_laplacian_pyramid(variables) in one launch (reference strotss_utils.py:159-163); None when the pyramid's
    shape is not one the kernel takes (the caller folds level by level)."""
    p = _hip.PyramidT()
    p.n_levels = len(variables)
    for k, v in enumerate(variables):
        require(v, "pyramid level")
        h, w, c = hwc(v)
        if c != 3 or len(variables) > 8:
            return None
        p.h[k], p.w[k], p.var[k] = h, w, v.data_ptr()
    rc = _hip.lib().strotss_fold_pyramid(C.byref(p), ptr(out), stream_ptr())
    if rc == -3:          # STROTSS_ERANGE: not a shrinking, at-least-halving pyramid
        return None
    check(rc, "fold_pyramid")
    return out


def fold_pyramid_adjoint(gvars: Sequence[torch.Tensor]) -> bool:
    """gvars[k] = resize_bilinear_adjoint(gvars[k-1]) for k >= 1 (gvars[0] = gradient of the folded image), two levels per
    launch where the pyramid halves; False when the tensors are not a 3-channel pyramid of at most 8 levels (caller: level by
    level)."""
    if len(gvars) < 2 or len(gvars) > 8 or any(int(g.shape[-1]) != 3 for g in gvars):
        return False
    p = _hip.PyramidT()
    p.n_levels = len(gvars)
    for k, g in enumerate(gvars):
        require(g, "pyramid gradient")
        p.h[k], p.w[k], p.var[k] = int(g.shape[-3]), int(g.shape[-2]), g.data_ptr()
    check(_hip.lib().strotss_fold_pyramid_adjoint(C.byref(p), stream_ptr()), "fold_pyramid_adjoint")
    return True


def flow_warp(prev: torch.Tensor, flow_b: torch.Tensor, flow_f: Optional[torch.Tensor] = None,
              warped: Optional[torch.Tensor] = None, certainty: Optional[torch.Tensor] = None):
    """(warped, certainty) of the temporal term (strotss_flow_warp): prev (1, h, w, c) or (h, w, c)
    warped along the backward flow (h, w, 2), certainty (h, w) in {0, 1}; flow_f (h, w, 2) or None (no disocclusion test)."""
    require(prev, "previous frame")
    require(flow_b, "backward flow")
    h, w, c = hwc(prev)
    assert tuple(flow_b.shape[-3:]) == (h, w, 2) and flow_b.numel() == 2 * h * w
    if flow_f is not None:
        require(flow_f, "forward flow")
        assert tuple(flow_f.shape[-3:]) == (h, w, 2) and flow_f.numel() == 2 * h * w
    if warped is None:
        warped = torch.empty_like(prev)
    if certainty is None:
        certainty = torch.empty((h, w), dtype=torch.float32, device=prev.device)
    require(warped, "warped frame")
    require(certainty, "certainty")
    assert warped.numel() == h * w * c and certainty.numel() == h * w
    check(_hip.lib().strotss_flow_warp(ptr(prev), h, w, c, ptr(flow_b), ptr(flow_f), ptr(warped), ptr(certainty),
                                       stream_ptr()), "flow_warp")
    return warped, certainty


def _zeroed_workspace(nbytes: int, device) -> torch.Tensor:
    """the allocator behind Workspaces.zeroed: `nbytes` (at least 16) of zeros; a ticketed reduction's counter returns to 0"""
    return torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def term_workspace(tag: str, h: int, w: int, device, ws: Optional["Workspaces"] = None, count: Optional[int] = None):
    """the zeroed workspace (Workspaces.zeroed of `ws`, None: the module-level instance) of a pixel-space term for (h, w): tag
    "temporal" (with `count` targets: the partials' layout depends on it), "detail", "tv" or "matting"; the library's bytes"""
    key = (int(h), int(w)) + (() if count is None else (int(count),))
    nb = getattr(_hip.lib(), f"strotss_{'temporal_multi' if tag == 'temporal' else tag}_workspace_bytes")(*key)
    if nb == 0:
        raise _hip.StrotssHipError(f"{tag} workspace: bad size {key}")
    return (ws or workspaces).zeroed(tag, key, int(nb), device)


def temporal_fwd_bwd(img: torch.Tensor, target: torch.Tensor, certainty: torch.Tensor, gscale: float, gimg: torch.Tensor,
                     loss_out: torch.Tensor, workspace: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None) -> None:
    """loss_out[0] = (1/(3hw)) sum_p certainty(p) |img(p) - target(p)|^2, gimg += gscale * dloss/dimg: temporal_multi_fwd_bwd
    with one target (its zeroed workspace, without an explicit one, is the "temporal" one of key (h, w, 1))"""
    temporal_multi_fwd_bwd(img, [target], [certainty], [gscale], gimg, loss_out, workspace, ws)


def temporal_long_certainty(stack: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the long-term certainties of one frame (strotss_temporal_long_certainty): stack (count, h, w),
    plane j the raw certainty of the j-th nearest earlier frame -> (count, h, w), plane j = max(c_j - sum_{k<j} c_k, 0)."""
    require(stack, "certainty stack")
    if stack.dim() != 3 or not 1 <= int(stack.shape[0]) <= _hip.MAX_TEMPORAL:
        raise ValueError(f"certainty stack of shape {tuple(stack.shape)}: expected (1..{_hip.MAX_TEMPORAL}, h, w)")
    count, h, w = (int(s) for s in stack.shape)
    if out is None:
        out = torch.empty_like(stack)
    require(out, "combined certainties")
    assert out.numel() == stack.numel()
    check(_hip.lib().strotss_temporal_long_certainty(ptr(stack), count, h, w, ptr(out), stream_ptr()),
          "temporal_long_certainty")
    return out


def temporal_multi_fwd_bwd(img: torch.Tensor, targets: Sequence[torch.Tensor], certainties: Sequence[torch.Tensor],
                           gscales: Sequence[float], gimg: torch.Tensor, loss_out: torch.Tensor,
                           workspace: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None) -> None:
    """loss_out[j] = (1/(3hw)) sum_p certainties[j](p) |img(p) - targets[j](p)|^2 for every j, gimg += sum_j gscales[j] *
    dloss_j/dimg in ONE launch (strotss_temporal_multi_fwd_bwd; img, targets, gimg (h, w, 3) or (1, h, w, 3), certainties
    (h, w)).  workspace: an explicit zeroed one of the library's size, or None for term_workspace's of `ws`."""
    count = len(targets)
    if not 1 <= count <= _hip.MAX_TEMPORAL or len(certainties) != count or len(gscales) != count:
        raise ValueError(f"{count} temporal targets, {len(certainties)} certainties, {len(gscales)} weights: expected "
                         f"1..{_hip.MAX_TEMPORAL} of each")
    for t, name in ((img, "image"), (gimg, "pixel gradient"), (loss_out, "temporal losses")):
        require(t, name)
    h, w, c = hwc(img)
    assert c == 3 and gimg.numel() == 3 * h * w and loss_out.numel() >= count
    workspace = term_workspace("temporal", h, w, img.device, ws, count) if workspace is None else workspace
    s = _hip.TemporalSetT()
    s.count = count
    for j, (tg, ce, g) in enumerate(zip(targets, certainties, gscales)):
        require(tg, f"temporal target {j}")
        require(ce, f"certainty {j}")
        assert tg.numel() == 3 * h * w and ce.numel() == h * w
        s.target[j], s.certainty[j], s.gscale[j] = tg.data_ptr(), ce.data_ptr(), float(g)
    check(_hip.lib().strotss_temporal_multi_fwd_bwd(ptr(img), C.byref(s), h, w, ptr(gimg), ptr(loss_out), ptr(workspace),
                                                    stream_ptr()), "temporal_multi_fwd_bwd")


TV_EPS = 1.0 / 255.0        # the total variation's smoothing: one grey level; a convention, not tuned


def pooled_shape(h: int, w: int, p: int) -> Tuple[int, int]:
    """(ceil(h / p), ceil(w / p)): the cell grid of pool size p"""
    return -(-int(h) // int(p)), -(-int(w) // int(p))


def check_detail_pools(pools) -> List[int]:
    """the pool sizes of the detail term as a list: 1..MAX_DETAIL_POOLS distinct values of DETAIL_POOLS, ascending
    (ValueError otherwise)"""
    ps = list(pools) if isinstance(pools, (list, tuple)) else None
    if ps is None or not 1 <= len(ps) <= _hip.MAX_DETAIL_POOLS or \
            any(isinstance(p, bool) or not isinstance(p, (int, np.integer)) or int(p) not in _hip.DETAIL_POOLS for p in ps) or \
            any(int(b) <= int(a) for a, b in zip(ps, ps[1:])):
        raise ValueError(f"detail pool sizes must be 1..{_hip.MAX_DETAIL_POOLS} distinct values of {_hip.DETAIL_POOLS}, "
                         f"ascending, got {pools!r}")
    return [int(p) for p in ps]


def pool_mean(img: torch.Tensor, p: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """P_p(img) (strotss_pool_mean): img (h, w, ch) or (1, h, w, ch), ch 1 or 3 -> (hp, wp, ch), every
    cell the mean of the pixels it covers"""
    require(img, "image to pool")
    h, w, ch = hwc(img)
    assert img.numel() == h * w * ch
    hp, wp = pooled_shape(h, w, p)
    if out is None:
        out = torch.empty((hp, wp, ch), dtype=torch.float32, device=img.device)
    require(out, "pooled image")
    assert out.numel() == hp * wp * ch
    check(_hip.lib().strotss_pool_mean(ptr(img), h, w, ch, int(p), ptr(out), stream_ptr()), "pool_mean")
    return out


def detail_fwd_bwd(img: torch.Tensor, pools: Sequence[int], contents: Sequence[torch.Tensor],
                   weights: Sequence[Optional[torch.Tensor]], gscales: Sequence[float], gimg: torch.Tensor,
                   loss_out: torch.Tensor, workspace: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None) -> None:
    """loss_out[j] = the Laplacian detail term of pool size pools[j], gimg += sum_j gscales[j] * dloss_j/dimg
    (strotss_detail_fwd_bwd; img, gimg (h, w, 3) or (1, h, w, 3), contents[j] = pool_mean(content, pools[j]), weights[j] the
    (hp, wp) cell weights or None).  workspace: as temporal_multi_fwd_bwd's."""
    count = len(pools)
    if not 1 <= count <= _hip.MAX_DETAIL_POOLS or len(contents) != count or len(weights) != count or len(gscales) != count:
        raise ValueError(f"{count} pool sizes, {len(contents)} pooled contents, {len(weights)} cell weights, {len(gscales)} "
                         f"weights: expected 1..{_hip.MAX_DETAIL_POOLS} of each")
    for t, name in ((img, "image"), (gimg, "pixel gradient"), (loss_out, "detail losses")):
        require(t, name)
    h, w, c = hwc(img)
    assert c == 3 and gimg.numel() == 3 * h * w and loss_out.numel() >= count
    workspace = term_workspace("detail", h, w, img.device, ws) if workspace is None else workspace
    s = _hip.DetailSetT()
    s.count = count
    for j, (p, ct, wt, g) in enumerate(zip(pools, contents, weights, gscales)):
        require(ct, f"pooled content {j}")
        s.pool[j], s.content[j], s.gscale[j] = int(p), ct.data_ptr(), float(g)
        if int(p) in _hip.DETAIL_POOLS:          # (another value: the library refuses it)
            hp, wp = pooled_shape(h, w, p)
            assert ct.numel() == 3 * hp * wp
        if wt is not None:
            require(wt, f"cell weights {j}")
            assert int(p) not in _hip.DETAIL_POOLS or wt.numel() == hp * wp
            s.weight[j] = wt.data_ptr()
    check(_hip.lib().strotss_detail_fwd_bwd(ptr(img), h, w, C.byref(s), ptr(gimg), ptr(loss_out), ptr(workspace),
                                            stream_ptr()), "detail_fwd_bwd")


def tv_fwd_bwd(img: torch.Tensor, gscale: float, gimg: torch.Tensor, loss_out: torch.Tensor,
               workspace: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None, eps: float = TV_EPS) -> None:
    """loss_out[0] = (1/(3hw)) sum (sqrt(dx^2 + dy^2 + eps^2) - eps), gimg += gscale * dloss/dimg (strotss_tv_fwd_bwd; img,
    gimg (h, w, 3) or (1, h, w, 3)).  workspace: as temporal_multi_fwd_bwd's."""
    for t, name in ((img, "image"), (gimg, "pixel gradient"), (loss_out, "tv loss")):
        require(t, name)
    h, w, c = hwc(img)
    assert c == 3 and gimg.numel() == 3 * h * w
    workspace = term_workspace("tv", h, w, img.device, ws) if workspace is None else workspace
    check(_hip.lib().strotss_tv_fwd_bwd(ptr(img), h, w, float(eps), float(gscale), ptr(gimg), ptr(loss_out), ptr(workspace),
                                        stream_ptr()), "tv_fwd_bwd")


# ------------------------------------------------------------------ photorealism term
def matting_prepare(guide: torch.Tensor, radius: int, eps: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the window statistics of the (h, w, 3) guide for matting_fwd_bwd (strotss_matting_prepare, one launch, once per
    scale): (9, h, w) float32, planes 0..2 the clipped window's mean, planes 3..8 the entries 00 01 02 11 12 22 of the
    inverse of cov_w(guide) + eps Id, computed in float64.  The library refuses a radius outside 1..4 and an eps outside
    [1e-4, 1]."""
    h, w = _rgb_image(guide, "guide")
    if out is None:
        out = torch.empty((9, h, w), dtype=torch.float32, device=guide.device)
    require(out, "window statistics")
    assert 4 * out.numel() == _hip.lib().strotss_matting_stats_bytes(h, w)
    check(_hip.lib().strotss_matting_prepare(ptr(guide), h, w, int(radius), float(eps), ptr(out), stream_ptr()),
          "matting_prepare")
    return out


def matting_fwd_bwd(img: torch.Tensor, guide: torch.Tensor, stats: torch.Tensor, radius: int, gscale: float,
                    gimg: torch.Tensor, loss_out: torch.Tensor, workspace: Optional[torch.Tensor] = None,
                    ws: Optional["Workspaces"] = None) -> None:
    """loss_out[0] = L_photo = (1/(3hw)) sum_i N_i sum_c img_c(i) (img_c(i) - q_c(i)), q the guided filter of img by guide
    over windows of radius `radius`; gimg += gscale * dL_photo/dimg (strotss_matting_fwd_bwd, one launch; img, guide, gimg
    (h, w, 3) or (1, h, w, 3), stats = matting_prepare(guide, radius, eps)).  workspace: as temporal_multi_fwd_bwd's."""
    for t, name in ((img, "image"), (guide, "guide"), (stats, "window statistics"), (gimg, "pixel gradient"),
                    (loss_out, "photo loss")):
        require(t, name)
    h, w, c = hwc(img)
    assert c == 3 and guide.numel() == 3 * h * w and gimg.numel() == 3 * h * w and stats.numel() == 9 * h * w
    workspace = term_workspace("matting", h, w, img.device, ws) if workspace is None else workspace
    check(_hip.lib().strotss_matting_fwd_bwd(ptr(img), ptr(guide), ptr(stats), h, w, int(radius), float(gscale), ptr(gimg),
                                             ptr(loss_out), ptr(workspace), stream_ptr()), "matting_fwd_bwd")


def flow_params(**overrides) -> "_hip.FlowParamsT":
    """strotss_flow_params_t with the library's defaults (strotss_flow_default_params; needs no GPU), fields overridden by
    name: alpha2, warps, iters, min_side, max_levels, iters_per_launch"""
    p = _hip.FlowParamsT()
    _hip.load_library().strotss_flow_default_params(C.byref(p))
    names = {f[0] for f in _hip.FlowParamsT._fields_}
    for key, val in overrides.items():
        if key not in names:
            raise ValueError(f"unknown flow parameter {key!r}: expected one of {sorted(names)}")
        setattr(p, key, val)
    return p


FLOW_MATCH_MAX_RADIUS = 4          # STROTSS_FLOW_MATCH_MAX_RADIUS


FLOW_ROBUST_FIELDS = ("alpha", "eps_d", "eps_s", "outer")          # strotss_flow_robust_params_t
FLOW_ROBUST_MAX_OUTER = 8                                           # STROTSS_FLOW_ROBUST_MAX_OUTER


def flow_robust_params(robust) -> Optional["_hip.FlowRobustParamsT"]:
    """strotss_flow_robust_params_t of `robust`: None -> None (the quadratic flow); a dict with any of alpha, eps_d, eps_s,
    outer (the others at the library's defaults, strotss_flow_robust_default_params; {} = all defaults), a tuple of the four
    in that order, or the struct itself.  ValueError for another key or length, a value that is not finite and > 0, an outer
    outside 1..8 (that outer divides iters is the library's check: it knows the flow parameters)."""
    if robust is None or isinstance(robust, _hip.FlowRobustParamsT):
        return robust
    p = _hip.FlowRobustParamsT()
    _hip.load_library().strotss_flow_robust_default_params(C.byref(p))
    if isinstance(robust, dict):
        unknown = sorted(set(robust) - set(FLOW_ROBUST_FIELDS))
        if unknown:
            raise ValueError(f"unknown robust flow parameter {unknown[0]!r}: expected one of {list(FLOW_ROBUST_FIELDS)}")
        items = robust.items()
    elif isinstance(robust, (tuple, list)) and len(robust) == len(FLOW_ROBUST_FIELDS):
        items = zip(FLOW_ROBUST_FIELDS, robust)
    else:
        raise ValueError(f"robust = {robust!r}: expected None, a dict or a tuple of {list(FLOW_ROBUST_FIELDS)}")
    for key, val in items:
        if key == "outer":
            if isinstance(val, bool) or int(val) != val or not 1 <= int(val) <= FLOW_ROBUST_MAX_OUTER:
                raise ValueError(f"robust flow: outer = {val!r}, expected a whole number in 1..{FLOW_ROBUST_MAX_OUTER}")
            p.outer = int(val)
        else:
            val = float(val)
            if not (val == val and 0.0 < val < float("inf")):
                raise ValueError(f"robust flow: {key} = {val}, expected a finite value > 0")
            setattr(p, key, val)
    return p


def optical_flow(frame_a: torch.Tensor, frame_b: torch.Tensor, params: Optional["_hip.FlowParamsT"] = None,
                 out: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None, match_radius: int = 0,
                 robust=None) -> torch.Tensor:
    """the dense optical flow (h, w, 2) = (u, v) with frame_a(p) ~ frame_b(p + flow(p)) (strotss_optical_flow, DESIGN.md
    section 14): frames (h, w, 3) or (1, h, w, 3) RGB in [0, 1]; params from flow_params(), None = the defaults.  The
    backward flow of frame t for strotss_flow_warp is optical_flow(frame_t, frame_{t-j}), the forward one
    optical_flow(frame_{t-j}, frame_t).  match_radius R in 1..4: with the patch-matching stage at every level
    (strotss_optical_flow_match); 0: without, the same launches as ever.  robust: None, or what
    flow_robust_params takes: the robust solver (strotss_optical_flow_robust); None is the call it
    always was.  The workspace is a buffer of this call's own, or grow-only scratch of `ws` when one is given."""
    require(frame_a, "frame a")
    require(frame_b, "frame b")
    h, w, c = hwc(frame_a)
    if c != 3 or frame_a.numel() != 3 * h * w or tuple(frame_b.shape[-3:]) != (h, w, 3) or frame_b.numel() != 3 * h * w:
        raise ValueError(f"frames of shape {tuple(frame_a.shape)} and {tuple(frame_b.shape)}: expected two (h, w, 3) images "
                         f"of one size")
    match_radius = int(match_radius)
    if not 0 <= match_radius <= FLOW_MATCH_MAX_RADIUS:
        raise ValueError(f"optical_flow: match_radius {match_radius}, expected 0 (no stage) .. {FLOW_MATCH_MAX_RADIUS}")
    lib = _hip.lib()
    pp = None if params is None else C.byref(params)
    rp = flow_robust_params(robust)
    nb = int(lib.strotss_flow_workspace_bytes(h, w, pp) if rp is None
             else lib.strotss_flow_robust_workspace_bytes(h, w, pp, C.byref(rp)))
    if nb == 0:
        raise _hip.StrotssHipError(f"optical_flow: bad size {h} x {w} or parameters")
    if out is None:
        out = torch.empty((h, w, 2), dtype=torch.float32, device=frame_a.device)
    require(out, "flow")
    assert out.numel() == 2 * h * w
    workspace = (torch.empty(nb, dtype=torch.uint8, device=frame_a.device) if ws is None
                 else ws.get("optical_flow", nb, frame_a.device))
    if rp is None:
        check(lib.strotss_optical_flow_match(ptr(frame_a), ptr(frame_b), h, w, pp, match_radius, ptr(out), ptr(workspace), nb,
                                             stream_ptr()), "optical_flow")
    else:
        check(lib.strotss_optical_flow_robust(ptr(frame_a), ptr(frame_b), h, w, pp, C.byref(rp), match_radius, ptr(out),
                                              ptr(workspace), nb, stream_ptr()), "optical_flow")
    return out


def flow_robust_stage(coef: torch.Tensor, u: torch.Tensor, v: torch.Tensor, robust=None, sweeps: int = 8,
                      iters_per_launch: int = 1):
    """one weight update of the robust flow on its own (strotss_flow_robust_stage): coef (h, w, 4) =
    {Ix, Iy, c, unused} and the flow planes u, v (h, w) -> (u', v', s (h, w), gk (h, w, 2) = {1 / G, k}) after `sweeps`
    weighted sweeps in launches of iters_per_launch"""
    for t, name in ((coef, "coef"), (u, "u"), (v, "v")):
        require(t, name)
    if u.dim() != 2 or tuple(v.shape) != tuple(u.shape) or tuple(coef.shape) != tuple(u.shape) + (4,):
        raise ValueError(f"flow_robust_stage: coef {tuple(coef.shape)}, u {tuple(u.shape)}, v {tuple(v.shape)}: expected "
                         f"(h, w, 4) and two (h, w) planes")
    h, w = int(u.shape[0]), int(u.shape[1])
    rp = flow_robust_params({} if robust is None else robust)
    uo, vo, s = torch.empty_like(u), torch.empty_like(v), torch.empty_like(u)
    gk = torch.empty((h, w, 2), dtype=torch.float32, device=u.device)
    tmp = torch.empty((2, h, w), dtype=torch.float32, device=u.device)
    check(_hip.lib().strotss_flow_robust_stage(ptr(coef), ptr(u), ptr(v), h, w, C.byref(rp), int(sweeps), int(iters_per_launch),
                                               ptr(uo), ptr(vo), ptr(s), ptr(gk), ptr(tmp), stream_ptr()),
          "flow_robust_stage")
    return uo, vo, s, gk


def flow_match_stage(a: torch.Tensor, b: torch.Tensor, u: torch.Tensor, v: torch.Tensor,
                     match_radius: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """the patch-matching stage alone (strotss_flow_match_stage): grey planes a, b and the flow
    planes u, v, all (h, w) float32 -> new (u, v), each pixel's flow moved by the whole offset in [-R, R]^2 whose 5 x 5
    window matches best (d = 0 wins ties)"""
    for t, name in ((a, "a"), (b, "b"), (u, "u"), (v, "v")):
        require(t, name)
        if t.dim() != 2 or tuple(t.shape) != tuple(a.shape):
            raise ValueError(f"flow_match_stage: {name} of shape {tuple(t.shape)}, expected four (h, w) planes of one size")
    match_radius = int(match_radius)
    if not 1 <= match_radius <= FLOW_MATCH_MAX_RADIUS:
        raise ValueError(f"flow_match_stage: match_radius {match_radius}, expected 1 .. {FLOW_MATCH_MAX_RADIUS}")
    h, w = int(a.shape[0]), int(a.shape[1])
    uo, vo = torch.empty_like(u), torch.empty_like(v)
    check(_hip.lib().strotss_flow_match_stage(ptr(a), ptr(b), h, w, ptr(u), ptr(v), match_radius, ptr(uo), ptr(vo),
                                              stream_ptr()), "flow_match_stage")
    return uo, vo


# ------------------------------------------------------------------ colour preservation
def _rgb_image(t: torch.Tensor, name: str) -> Tuple[int, int]:
    """(h, w) of an (h, w, 3) or (1, h, w, 3) image on the device; ValueError for another shape"""
    require(t, name)
    if t.dim() not in (3, 4) or int(t.shape[-1]) != 3 or t.numel() != 3 * int(t.shape[-3]) * int(t.shape[-2]):
        raise ValueError(f"{name} of shape {tuple(t.shape)}: expected (h, w, 3) or (1, h, w, 3)")
    return int(t.shape[-3]), int(t.shape[-2])


def _weight_plane(weight: Optional[torch.Tensor], h: int, w: int, name: str) -> Optional[torch.Tensor]:
    if weight is None:
        return None
    require(weight, name)
    if weight.numel() != h * w or tuple(weight.shape[:2]) != (h, w):
        raise ValueError(f"{name} of shape {tuple(weight.shape)}: expected ({h}, {w}) or ({h}, {w}, 1)")
    return weight


def color_stats(img: torch.Tensor, weight: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the ten float64 sums (W, S_0, S_1, S_2, S_00, S_01, S_02, S_11, S_12, S_22) of an (h, w, 3) image under an optional
    (h, w) weight plane, on the device (strotss_color_stats; one launch, the same bits on every run).  The workspace is
    one per device and size (Workspaces.zeroed)."""
    h, w = _rgb_image(img, "image")
    weight = _weight_plane(weight, h, w, "weight plane")
    lib = _hip.lib()
    nb = int(lib.strotss_color_stats_workspace_bytes(h, w))
    if nb == 0:
        raise _hip.StrotssHipError(f"color_stats: bad size {h} x {w}")
    workspace = (ws or workspaces).zeroed("color_stats", (h, w), nb, img.device)
    if out is None:
        out = torch.empty(10, dtype=torch.float64, device=img.device)
    assert out.is_cuda and out.dtype == torch.float64 and out.is_contiguous() and out.numel() == 10
    check(lib.strotss_color_stats(ptr(img), ptr(weight), h, w, ptr(out), ptr(workspace), stream_ptr()), "color_stats")
    return out


def color_affine(img: torch.Tensor, A, b, weight: Optional[torch.Tensor] = None,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out(p) = A img(p) + b where weight(p) != 0 (None: everywhere), img(p) elsewhere (strotss_color_affine): A nine and b
    three host values, rounded to float32 here; out may be img."""
    h, w = _rgb_image(img, "image")
    weight = _weight_plane(weight, h, w, "weight plane")
    a9 = (C.c_float * 9)(*np.asarray(A, dtype=np.float64).reshape(9).astype(np.float32).tolist())
    b3 = (C.c_float * 3)(*np.asarray(b, dtype=np.float64).reshape(3).astype(np.float32).tolist())
    if out is None:
        out = torch.empty_like(img)
    require(out, "recoloured image")
    assert out.numel() == img.numel()
    check(_hip.lib().strotss_color_affine(ptr(img), ptr(weight), h, w, a9, b3, ptr(out), stream_ptr()), "color_affine")
    return out


def luma_merge(result: torch.Tensor, content: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out_ch = content_ch + (Y(result) - Y(content)) (strotss_luma_merge): two images of one size; out may be result."""
    h, w = _rgb_image(result, "result")
    if _rgb_image(content, "content") != (h, w):
        raise ValueError(f"result of shape {tuple(result.shape)} and content of shape {tuple(content.shape)} differ in size")
    if out is None:
        out = torch.empty_like(result)
    require(out, "merged image")
    assert out.numel() == result.numel()
    check(_hip.lib().strotss_luma_merge(ptr(result), ptr(content), h, w, ptr(out), stream_ptr()), "luma_merge")
    return out


# ------------------------------------------------------------------ colour distribution transfer
_transfer_ws = {}      # not scratch: the typed running state (histogram, table) of the one transfer at a time


def _bases(bases, name: str = "bases"):
    """(n, 3, 3) or (3, 3) host values -> (n, the n * 9 floats as a ctypes array), rounded to float32 here"""
    b = np.asarray(bases, dtype=np.float64)
    if b.ndim == 2:
        b = b[None]
    if b.ndim != 3 or b.shape[1:] != (3, 3) or b.shape[0] < 1:
        raise ValueError(f"{name} of shape {b.shape}: expected (n, 3, 3) or (3, 3)")
    flat = b.astype(np.float32).reshape(-1)
    return int(b.shape[0]), (C.c_float * flat.size)(*flat.tolist())


def _counts(t: torch.Tensor, shape: Tuple[int, ...], name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous()) or tuple(t.shape) != shape:
        raise _hip.StrotssHipError(f"{name} must be a contiguous int32 CUDA/HIP tensor of shape {shape}, got {t.dtype} "
                                   f"{t.device} {tuple(t.shape)}")
    return t


def color_transfer_workspace(device, bins: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(hist (3, bins) int32, table (3, bins + 1) float32): the running histogram of the moved style and the current
    table of a transfer, a module-level pair per device and bin count (one transfer at a time)."""
    key = (str(canonical_device(device)), int(bins))
    ws = _transfer_ws.get(key)
    if ws is None:
        ws = _transfer_ws[key] = (torch.zeros((3, bins), dtype=torch.int32, device=device),
                                  torch.zeros((3, bins + 1), dtype=torch.float32, device=device))
    return ws


def color_hist(img: torch.Tensor, bases, bins: int, weight: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(n, 3, bins) int32 (the bits of uint32 counts): the histograms of the projections of the pixels whose weight is != 0
    (None: all) on the three axes of each of the n bases (strotss_color_hist: one kernel launch for all of them)."""
    h, w = _rgb_image(img, "image")
    weight = _weight_plane(weight, h, w, "weight plane")
    n, flat = _bases(bases)
    if out is None:
        out = torch.empty((n, 3, int(bins)), dtype=torch.int32, device=img.device)
    _counts(out, (n, 3, int(bins)), "histograms")
    check(_hip.lib().strotss_color_hist(ptr(img), ptr(weight), h, w, flat, n, int(bins), ptr(out), stream_ptr()),
          "color_hist")
    return out


def color_transfer_table(hist_src: torch.Tensor, hist_dst: torch.Tensor, basis, bins: int,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """(3, bins + 1) float32: per axis of `basis` the monotone map from the source's bin edges to the target's axis that
    matches the two (3, bins) histograms (strotss_color_transfer_table)."""
    n, flat = _bases(basis, "basis")
    if n != 1:
        raise ValueError("color_transfer_table takes one basis")
    _counts(hist_src, (3, int(bins)), "source histogram")
    _counts(hist_dst, (3, int(bins)), "target histogram")
    if out is None:
        out = torch.empty((3, int(bins) + 1), dtype=torch.float32, device=hist_src.device)
    require(out, "transfer table")
    assert tuple(out.shape) == (3, int(bins) + 1)
    check(_hip.lib().strotss_color_transfer_table(ptr(hist_src), ptr(hist_dst), flat, int(bins), ptr(out), stream_ptr()),
          "color_transfer_table")
    return out


def color_transfer_apply(img: torch.Tensor, basis, table: torch.Tensor, bins: int, weight: Optional[torch.Tensor] = None,
                         out: Optional[torch.Tensor] = None, next_basis=None,
                         next_hist: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = img moved along the three axes of `basis` by `table` where weight != 0 (None: everywhere), img elsewhere
    (strotss_color_transfer_apply; out may be img).  next_basis and next_hist ((3, bins) int32), both or neither: the same
    launch leaves the histogram of the moved pixels on next_basis in next_hist."""
    h, w = _rgb_image(img, "image")
    weight = _weight_plane(weight, h, w, "weight plane")
    n, flat = _bases(basis, "basis")
    if n != 1:
        raise ValueError("color_transfer_apply takes one basis")
    require(table, "transfer table")
    assert tuple(table.shape) == (3, int(bins) + 1)
    if (next_basis is None) != (next_hist is None):
        raise ValueError("color_transfer_apply: next_basis and next_hist come together")
    nflat = None
    if next_basis is not None:
        n, nflat = _bases(next_basis, "next basis")
        if n != 1:
            raise ValueError("color_transfer_apply takes one next basis")
        _counts(next_hist, (3, int(bins)), "next histogram")
    if out is None:
        out = torch.empty_like(img)
    require(out, "moved image")
    assert out.numel() == img.numel()
    check(_hip.lib().strotss_color_transfer_apply(ptr(img), ptr(weight), h, w, flat, ptr(table), int(bins), ptr(out), nflat,
                                                  ptr(next_hist), stream_ptr()), "color_transfer_apply")
    return out


# ------------------------------------------------------------------ photo smoothing
def guided_smooth(img: torch.Tensor, guide: torch.Tensor, radius: int, eps: float,
                  out: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None) -> torch.Tensor:
    """the guided filter of an (h, w, 3) image with `guide` (the same size) as colour guide, windows of radius `radius`
    clipped to the image, regulariser `eps` at its float32 value (strotss_guided_smooth; four launches on the current
    stream, the same bits on every run).  out may be img, not guide.  The workspace (216 bytes per pixel) is grow-only
    scratch of `ws`; the library refuses a radius outside 1..64 and an eps outside [1e-4, 1]."""
    h, w = _rgb_image(img, "image")
    if _rgb_image(guide, "guide") != (h, w):
        raise ValueError(f"image of shape {tuple(img.shape)} and guide of shape {tuple(guide.shape)} differ in size")
    lib = _hip.lib()
    nb = int(lib.strotss_guided_smooth_workspace_bytes(h, w, 1))        # the size does not depend on the radius
    if nb == 0:
        raise _hip.StrotssHipError(f"guided_smooth: bad size {h} x {w}")
    workspace = (ws or workspaces).get("guided_smooth", nb, img.device)
    if out is None:
        out = torch.empty_like(img)
    require(out, "smoothed image")
    assert out.numel() == img.numel()
    check(lib.strotss_guided_smooth(ptr(img), ptr(guide), h, w, int(radius), float(eps), ptr(out), ptr(workspace),
                                    workspace.numel(), stream_ptr()), "guided_smooth")
    return out


# ------------------------------------------------------------------ guided upsampling
UPSAMPLE_MODES = {"guided": 0, "residual": 1}        # STROTSS_UPSAMPLE_GUIDED, STROTSS_UPSAMPLE_RESIDUAL


def guided_upsample(img: torch.Tensor, guide_lo: torch.Tensor, guide_hi: torch.Tensor, radius: int, eps: float, mode: str,
                    out: Optional[torch.Tensor] = None, ws: Optional["Workspaces"] = None) -> torch.Tensor:
    """the (h, w, 3) image brought to the size of `guide_hi` (H, W, 3), H >= h and W >= w, by the guided filter's window
    means at (h, w) (guide_lo: the guide at the image's size) interpolated and applied to guide_hi; mode "guided" or
    "residual" (that plus the interpolated img - filter(img)).  strotss_guided_upsample: five launches on the current
    stream, the same bits on every run.  out may overlap none of the inputs.  The workspace (280 bytes per low-resolution
    pixel) is grow-only scratch of `ws`; the library refuses what strotss_guided_smooth refuses, a smaller guide_hi and
    3 H W > INT_MAX."""
    h, w = _rgb_image(img, "image")
    if _rgb_image(guide_lo, "low-resolution guide") != (h, w):
        raise ValueError(f"image of shape {tuple(img.shape)} and guide of shape {tuple(guide_lo.shape)} differ in size")
    H, W = _rgb_image(guide_hi, "full-resolution guide")
    if mode not in UPSAMPLE_MODES:
        raise ValueError(f"upsampling mode {mode!r}: expected one of {tuple(UPSAMPLE_MODES)}")
    lib = _hip.lib()
    nb = int(lib.strotss_guided_upsample_workspace_bytes(h, w, 1))      # the size does not depend on the radius
    if nb == 0:
        raise _hip.StrotssHipError(f"guided_upsample: bad size {h} x {w}")
    workspace = (ws or workspaces).get("guided_upsample", nb, img.device)
    if out is None:
        out = torch.empty_like(guide_hi)
    require(out, "upsampled image")
    assert out.numel() == guide_hi.numel()
    check(lib.strotss_guided_upsample(ptr(img), ptr(guide_lo), h, w, ptr(guide_hi), H, W, int(radius), float(eps),
                                      UPSAMPLE_MODES[mode], ptr(out), ptr(workspace), workspace.numel(), stream_ptr()),
          "guided_upsample")
    return out


# ------------------------------------------------------------------ detail map
def detail_map(img: torch.Tensor, radius: Optional[int] = None, gain: float = 2.0, floor: float = 0.25, ws=None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """the (h, w) float32 detail map of an (h, w, 3) image in [floor, 1]: the root of the windowed mean gradient energy of
    its luma over gain times that root's image mean, clamped at 1 (strotss_detail_map; three launches on the current stream,
    the same bits on every run).  radius None: max(1, longer side // 64), at most 64.  The workspace (8 bytes per pixel) is
    one per device and size (Workspaces.zeroed); the library refuses a radius outside 1..64, a gain that is not finite or
    <= 0 and a floor outside [0, 1]."""
    h, w = _rgb_image(img, "image")
    if radius is None:
        radius = max(1, min(64, max(h, w) // 64))
    lib = _hip.lib()
    nb = int(lib.strotss_detail_map_workspace_bytes(h, w))
    if nb == 0:
        raise _hip.StrotssHipError(f"detail_map: bad size {h} x {w}")
    workspace = (ws or workspaces).zeroed("detail_map", (h, w), nb, img.device)
    if out is None:
        out = torch.empty((h, w), dtype=torch.float32, device=img.device)
    require(out, "detail map")
    assert out.dtype == torch.float32 and out.numel() == h * w
    check(lib.strotss_detail_map(ptr(img), h, w, int(radius), float(gain), float(floor), ptr(out), ptr(workspace),
                                 stream_ptr()), "detail_map")
    return out


def resize_bilinear_adjoint(gout: torch.Tensor, ih: int, iw: int,
                            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    require(gout, "resize adjoint input")
    oh, ow, c = hwc(gout)
    if out is None:
        out = torch.empty((*gout.shape[:-3], ih, iw, c), dtype=torch.float32, device=gout.device)
    check(_hip.lib().strotss_resize_bilinear_adjoint(ptr(gout), oh, ow, c, ptr(out), ih, iw, stream_ptr()),
          "resize_bilinear_adjoint")
    return out


# ------------------------------------------------------------------ VGG layers
def _f3(v, default):
    return default if v is None else (C.c_float * 3)(*v)


def relu_bits_buffer(h: int, w: int, c: int, device) -> torch.Tensor:
    """Room for the sign words of an (h, w, c) activation: one int32 per (4x4 tile, channel), see include/strotss_hip.h."""
    return torch.empty(((h + 3) // 4) * ((w + 3) // 4), c, dtype=torch.int32, device=device)


def relu_bits(act, out=None):
    """Sign words of a finished activation tensor (1, h, w, c): byte r, bit q of word (tile, ch) = act[4ty+r, 4tx+q, ch] > 0."""
    require(act, "activation"); h, w, c = hwc(act)
    if out is None:
        out = relu_bits_buffer(h, w, c, act.device)
    check(_hip.lib().strotss_relu_bits(ptr(act), h, w, c, ptr(out), stream_ptr()), "relu_bits")
    return out


def conv3x3_c3_fwd(img, w_kio, bias, out=None, mean=None, std=None, relu_bits_out=None):
    require(img, "image"); h, w, c = hwc(img)
    assert c == 3
    cout = bias.numel()
    if out is None:
        out = torch.empty((1, h, w, cout), dtype=torch.float32, device=img.device)
    check(_hip.lib().strotss_conv3x3_c3_fwd(ptr(img), h, w, ptr(w_kio), ptr(bias), cout, _f3(mean, _MEAN3),
                                            _f3(std, _STD3), ptr(out), ptr(relu_bits_out), stream_ptr()), "conv3x3_c3_fwd")
    return out


def conv3x3_relu_fwd(x, w_tok, bias, out=None, pool_out=None, pool_code=None, ws=None):
    """pool_out (split-K layers only, conv3x3_direct_splits): the finish kernel also writes maxpool2_fwd(out) (+ pool_code)."""
    require(x, "conv input"); h, w, cin = hwc(x)
    cout = bias.numel()
    if out is None:
        out = torch.empty((1, h, w, cout), dtype=torch.float32, device=x.device)
    nb = _hip.lib().strotss_conv3x3_workspace_bytes(h, w, cin, cout)
    buf = (ws or workspaces).get("conv_splitk", nb, x.device) if nb else None
    if pool_out is not None:
        check(_hip.lib().strotss_conv3x3_relu_pool_fwd(ptr(x), h, w, cin, ptr(w_tok), ptr(bias), cout, ptr(out), ptr(pool_out),
                                                       ptr(pool_code), ptr(buf), nb, stream_ptr()), "conv3x3_relu_pool_fwd")
        return out
    check(_hip.lib().strotss_conv3x3_relu_fwd(ptr(x), h, w, cin, ptr(w_tok), ptr(bias), cout, ptr(out), ptr(buf), nb,
                                              stream_ptr()), "conv3x3_relu_fwd")
    return out


def conv3x3_direct_splits(h: int, w: int, cin: int, cout: int) -> bool:
    """True when a (h, w, cin -> cout) layer runs as the split-K direct kernel (which can also ADD to its output)."""
    return _hip.load_library().strotss_conv3x3_workspace_bytes(h, w, cin, cout) > 0


def conv3x3_dgrad_accumulates(h: int, w: int, cout: int, cin: int) -> bool:
    """True when conv3x3_dgrad(accumulate=True) launches for a (h, w, cout) gradient of a cin-channel input (the library's
    answer: its one-pass kernel of STROTSS_CONV_VARIANT=1 only overwrites).  No GPU needed."""
    return bool(_hip.load_library().strotss_conv3x3_dgrad_can_accumulate(h, w, cout, cin))


def conv3x3_dgrad(gout, w_tik, cin, act_in=None, out=None, accumulate=False, ws=None):
    require(gout, "conv grad"); h, w, cout = hwc(gout)
    if out is None:
        out = torch.empty((1, h, w, cin), dtype=torch.float32, device=gout.device)
    nb = _hip.lib().strotss_conv3x3_workspace_bytes(h, w, cout, cin)
    buf = (ws or workspaces).get("conv_splitk", nb, gout.device) if nb else None
    check(_hip.lib().strotss_conv3x3_dgrad(ptr(gout), h, w, cout, ptr(w_tik), cin, ptr(act_in), ptr(out), int(accumulate),
                                           ptr(buf), nb, stream_ptr()), "conv3x3_dgrad")
    return out


def conv3x3_dgrad_unpool(gout, w_tik, cin, pool_code, out_full, accumulate=False, ws=None):
    """Data gradient of a split-K layer whose input came from the 2x2/2 max-pool, written through the pool's adjoint:
    out_full (1, H, W, cin) (+)= maxpool2_bwd(code=pool_code, conv^T(gout)); the pooled gradient is never stored."""
    require(gout, "conv grad"); h, w, cout = hwc(gout)
    require(out_full, "gradient in front of the pool"); fh, fw, fc = hwc(out_full)
    assert fc == cin and fh // 2 == h and fw // 2 == w, (out_full.shape, gout.shape, cin)
    nb = _hip.lib().strotss_conv3x3_workspace_bytes(h, w, cout, cin)
    buf = (ws or workspaces).get("conv_splitk", nb, gout.device) if nb else None
    check(_hip.lib().strotss_conv3x3_dgrad_unpool(ptr(gout), h, w, cout, ptr(w_tik), cin, ptr(pool_code), ptr(out_full), fh, fw,
                                                  int(accumulate), ptr(buf), nb, stream_ptr()), "conv3x3_dgrad_unpool")
    return out_full


def conv3x3_c3_dgrad(gout, w_tic, gimg=None, accumulate=False, std=None):
    require(gout, "conv grad"); h, w, cout = hwc(gout)
    if gimg is None:
        gimg = torch.empty((1, h, w, 3), dtype=torch.float32, device=gout.device)
        accumulate = False
    check(_hip.lib().strotss_conv3x3_c3_dgrad(ptr(gout), h, w, cout, ptr(w_tic), _f3(std, _STD3), ptr(gimg),
                                              int(accumulate), stream_ptr()), "conv3x3_c3_dgrad")
    return gimg


def _wino_ws(h, w, cin, cout, tile_m, device, ws=None):
    nb = _hip.lib().strotss_conv3x3_winograd_workspace_bytes(h, w, cin, cout, tile_m)
    return (ws or workspaces).get("winograd", nb, device), nb


def _tile_m(u: torch.Tensor) -> int:
    return {16: 2, 36: 4}[int(u.shape[0])]


def winograd_packed(u: torch.Tensor):
    """The fragment-major copy of a (36, rows, k) Winograd weight tensor for the fused kernel, or None where the fused
    kernel does not apply.  Made once and kept on `u` itself (the weights are frozen), so it lives as long as they do."""
    if not winograd_packed_wanted(int(u.shape[0]), int(u.shape[1]), int(u.shape[2])):
        return None
    up = getattr(u, "_winograd_packed", None)
    if up is None:
        require(u, "winograd weights")
        up = torch.empty_like(u)
        check(_hip.lib().strotss_conv3x3_winograd_pack(ptr(u), int(u.shape[1]), int(u.shape[2]), ptr(up), stream_ptr()),
              "conv3x3_winograd_pack")
        u._winograd_packed = up
    return up


def env_int(name: str, default: int) -> int:
    """A host-only switch, parsed as the library's getenv + atoi / atol parse theirs: `default` when unset, otherwise the
    leading integer (after white space, with an optional sign), 0 when there is none -- so "", "00" and "false" are 0."""
    import os
    import re
    v = os.environ.get(name)
    if v is None:
        return default
    m = re.match(r"[ \t\n\v\f\r]*([+-]?[0-9]+)", v)
    return int(m.group(1)) if m else 0


def winograd_x3_wanted(p: int, rows: int, k: int, h: int, w: int) -> bool:
    """Whether an (h, w) layer with (p, rows, k) Winograd weights gets x3 panels: exactly where the library, offered them
    next to the packed copy it would also be offered, answers with a bf16x3 GEMM route (csrc/winograd.hip winograd43_route,
    the function its launches dispatch on).  A question to the library, no policy of the host's; needs no GPU."""
    return p == 36 and _hip.load_library().strotss_conv3x3_winograd_route(
        h, w, k, rows, 4, int(winograd_packed_wanted(p, rows, k)), 1) in (3, 4)      # STROTSS_ROUTE_F4_X3_GEMM_128 / _64


def winograd_packed_wanted(p: int, rows: int, k: int) -> bool:
    return p == 36 and rows % 32 == 0 and k % 32 == 0


def winograd_x3(u: torch.Tensor, h: int, w: int):
    """The x3 panels (three bf16 planes per f32 weight, K-blocked; csrc/mfma_x3.h) of a (36, rows, k) Winograd weight
    tensor for the bf16x3 GEMM core, or None where the library would not use them for an (h, w) layer
    (`winograd_x3_wanted`).  Made once and kept on `u` itself, like the packed copy."""
    if not winograd_x3_wanted(int(u.shape[0]), int(u.shape[1]), int(u.shape[2]), h, w):
        return None
    up = getattr(u, "_winograd_x3", None)
    if up is None:
        require(u, "winograd weights")
        rows, k = int(u.shape[1]), int(u.shape[2])
        nb = _hip.lib().strotss_conv3x3_winograd_x3_bytes(rows, k)
        up = torch.empty(nb // 2, dtype=torch.bfloat16, device=u.device)
        check(_hip.lib().strotss_conv3x3_winograd_x3pack(ptr(u), rows, k, ptr(up), stream_ptr()), "conv3x3_winograd_x3pack")
        u._winograd_x3 = up
    return up


def conv3x3_winograd_fwd(x, u_pok, bias, out=None, pool_out=None, pool_code=None, relu_bits_out=None, ws=None):
    """u_pok: (16, cout, cin) -> F(2x2,3x3), (36, cout, cin) -> F(4x4,3x3).  pool_out: (1, h//2, w//2, cout) buffer
    that also receives the 2x2/2 max-pool of the result.  relu_bits_out (F(4x4) only): relu_bits_buffer that receives the
    sign words of the result, for the next layer's conv3x3_winograd_dgrad."""
    require(x, "conv input"); h, w, cin = hwc(x)
    cout = bias.numel()
    if out is None:
        out = torch.empty((1, h, w, cout), dtype=torch.float32, device=x.device)
    m = _tile_m(u_pok)
    assert u_pok.device == x.device, (u_pok.device, x.device)
    buf, nb = _wino_ws(h, w, cin, cout, m, x.device, ws)
    check(_hip.lib().strotss_conv3x3_winograd_fwd(ptr(x), h, w, cin, ptr(u_pok), ptr(winograd_packed(u_pok)),
                                                  ptr(winograd_x3(u_pok, h, w)), ptr(bias),
                                                  cout, m, ptr(out), ptr(pool_out), ptr(pool_code), ptr(relu_bits_out), ptr(buf), nb,
                                                  stream_ptr()),
          "conv3x3_winograd_fwd")
    return out


def conv3x3_winograd_dgrad(gout, u_pik, cin, act_in=None, out=None, relu_bits=None, accumulate=False, ws=None):
    """relu_bits (F(4x4) only): the sign words of the layer's input activation; the ReLU mask then comes from them instead of
    act_in (same result, 1/16 of the bytes)."""
    require(gout, "conv grad"); h, w, cout = hwc(gout)
    if out is None:
        out = torch.empty((1, h, w, cin), dtype=torch.float32, device=gout.device)
    m = _tile_m(u_pik)
    assert u_pik.device == gout.device, (u_pik.device, gout.device)
    buf, nb = _wino_ws(h, w, cout, cin, m, gout.device, ws)
    check(_hip.lib().strotss_conv3x3_winograd_dgrad(ptr(gout), h, w, cout, ptr(u_pik), ptr(winograd_packed(u_pik)),
                                                    ptr(winograd_x3(u_pik, h, w)), cin,
                                                    m, ptr(act_in), ptr(relu_bits), ptr(out), int(accumulate), ptr(buf), nb,
                                                    stream_ptr()),
          "conv3x3_winograd_dgrad")
    return out


def winograd_weights(g: torch.Tensor, tile_m: int = 2, device=None) -> torch.Tensor:
    """g: (N, K, 3, 3) kernel as [out-channel][in-channel][r][q] -> U (P, N, K) float32 with
    U[a*(m+2)+b] = (G g G^T)[a, b], computed in float64 on the device (P = 16 for tile_m = 2, 36 for tile_m = 4).
    `device`: where a host-held `g` goes (the model's device; default: the current one)."""
    if not g.is_cuda and torch.cuda.is_available():
        g = g.to(canonical_device(device if device is not None else "cuda"))
    g = g.float().contiguous()
    require(g, "conv kernel")
    n, k = int(g.shape[0]), int(g.shape[1])
    u = torch.empty(((tile_m + 2) ** 2, n, k), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):          # stream_ptr() is the CURRENT device's stream: make that device g's
        check(_hip.lib().strotss_conv3x3_winograd_weights(ptr(g), n, k, tile_m, ptr(u), stream_ptr()),
              "conv3x3_winograd_weights")
    return u


def maxpool2_fwd(x, out=None, code=None):
    """code: optional (1, h//2, w//2, c) uint8 buffer receiving the argmax codes for maxpool2_bwd."""
    require(x, "pool input"); h, w, c = hwc(x)
    if out is None:
        out = torch.empty((1, h // 2, w // 2, c), dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_maxpool2_fwd(ptr(x), h, w, c, ptr(out), ptr(code), stream_ptr()), "maxpool2_fwd")
    return out


def maxpool2_bwd(act, gout, out=None, code=None, accumulate=False):
    """With `code` (from the forward pass) the activations are not read.  accumulate: out += instead of out =."""
    require(act, "pool act"); require(gout, "pool grad"); h, w, c = hwc(act)
    if out is None:
        out = torch.empty_like(act)
        accumulate = False
    check(_hip.lib().strotss_maxpool2_bwd(ptr(act), h, w, c, ptr(gout), ptr(out), ptr(code), int(accumulate), stream_ptr()),
          "maxpool2_bwd")
    return out


# ------------------------------------------------------------------ hypercolumns
def map_divisors(shapes: Sequence[Tuple[int, int]]) -> List[List[float]]:
    """Divisor chain per map: reference nn/strotss_utils.py:31-37 (`indices /= y`, cumulative, the
    axis chosen once from whether log2 of the first shrunk height is an integer)."""
    import math
    chains, cur, index = [], [], None
    for i, (h, w) in enumerate(shapes):
        if i > 0 and h < shapes[i - 1][0]:
            if index is None:
                index = 0 if not (math.log2(h) % 1) else 1
            cur = cur + [shapes[i - 1][index] / shapes[i][index]]
        chains.append(list(cur))
    return chains


def hypercol_gather(maps: Sequence[torch.Tensor], idx: torch.Tensor, bilinear: bool,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """-> (pad32(n), pad32(D)) feature buffer, rows >= n and columns >= D zero."""
    require(idx, "indices")
    n = idx.shape[0]
    d = sum(int(m.shape[-1]) for m in maps)
    if out is None:
        out = torch.zeros((pad32(n), pad32(d)), dtype=torch.float32, device=idx.device)
    mt = _hip.make_maps(maps, map_divisors([hwc(m)[:2] for m in maps]))
    check(_hip.lib().strotss_hypercol_gather(C.byref(mt), ptr(idx), n, int(bilinear), ptr(out),
                                             out.shape[1], stream_ptr()), "hypercol_gather")
    return out


def hypercol_scatter(maps: Sequence[torch.Tensor], gmaps: Sequence[Optional[torch.Tensor]],
                     idx: torch.Tensor, gfeat: torch.Tensor, relu_mask_from: int = 1,
                     map_begin: int = 0, map_end: Optional[int] = None, maps_t=None):
    """gmaps[k] += adjoint-gather of gfeat's columns of map k, for k in [map_begin, map_end)
    (float atomics).  `maps_t` may carry a prebuilt descriptor (engine hot loop)."""
    require(idx, "indices"); require(gfeat, "feature grads")
    if map_end is None:
        map_end = len(maps)
    mt = maps_t if maps_t is not None else _hip.make_maps(
        maps, map_divisors([hwc(m)[:2] for m in maps]), gmaps)
    check(_hip.lib().strotss_hypercol_scatter(C.byref(mt), ptr(idx), idx.shape[0], ptr(gfeat),
                                              gfeat.shape[1], relu_mask_from, map_begin, map_end,
                                              stream_ptr()), "hypercol_scatter")


def hypercol_scatter_plan(maps_t, idx: torch.Tensor, plan: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Plan of the deterministic scatter for one index set (all maps of `maps_t`); returns the plan buffer."""
    require(idx, "indices")
    nb = _hip.lib().strotss_hypercol_scatter_plan_bytes(int(maps_t.n_maps))
    if plan is None:
        plan = torch.empty(nb, dtype=torch.uint8, device=idx.device)
    check(_hip.lib().strotss_hypercol_scatter_plan(C.byref(maps_t), ptr(idx), idx.shape[0], plan.data_ptr(), plan.numel(),
                                                   stream_ptr()), "hypercol_scatter_plan")
    return plan


def hypercol_scatter_sorted(maps_t, plan: torch.Tensor, n: int, gfeat: torch.Tensor, relu_mask_from: int = 1,
                            map_begin: int = 0, map_end: Optional[int] = None):
    """gmaps[k] += adjoint-gather of gfeat's columns of map k, k in [map_begin, map_end), in plan order (no atomics)."""
    require(gfeat, "feature grads")
    if map_end is None:
        map_end = int(maps_t.n_maps)
    check(_hip.lib().strotss_hypercol_scatter_sorted(C.byref(maps_t), plan.data_ptr(), n, ptr(gfeat), gfeat.shape[1],
                                                     relu_mask_from, map_begin, map_end, stream_ptr()),
          "hypercol_scatter_sorted")


# ------------------------------------------------------------------ losses
def index_draw(h: int, w: int, sample_size: int, seed: int, counters: torch.Tensor, out_idx, masks=None, n_out=None,
               stride=None, general_path: bool = False) -> None:
    """One launch of strotss_index_draw (csrc/draw.hip; reference: Sampling._make_indices, strotss_utils.py:83-121): region r's
    next draw of its stream (draw number counters[r], advanced by `stride` afterwards) -> out_idx[r] (sample_size, 2) float32.
    masks: per region a (h, w) uint8 device tensor at THIS scale (nonzero = keep) or None; n_out: int32 (R,) or None.
    nn/rand.py:PhiloxStream(seed, t) is the host twin of draw number t."""
    check(_hip.lib().strotss_index_draw(C.byref(_draw_t(h, w, sample_size, seed, counters, out_idx, masks, n_out, stride,
                                                        general_path)), stream_ptr()), "index_draw")


def _draw_t(h, w, sample_size, seed, counters, out_idx, masks, n_out, stride, general_path) -> "_hip.DrawT":
    """the strotss_draw_t of index_draw and index_draw_weighted, its tensors checked"""
    from .strotss_utils import sampling_steps
    R = len(out_idx)
    assert 0 < R <= _hip.MAX_DRAW_REGIONS and counters.dtype == torch.int32 and counters.numel() >= R and counters.is_cuda
    d = _hip.DrawT()
    d.h, d.w = int(h), int(w)
    d.step_x, d.step_y = sampling_steps(int(h), int(w))
    d.sample_size, d.n_regions = int(sample_size), R
    d.seed_lo, d.seed_hi = int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF
    d.counter_stride = R if stride is None else int(stride)
    for r in range(R):
        o = out_idx[r]
        assert o.is_cuda and o.dtype == torch.float32 and o.is_contiguous() and o.numel() >= 2 * sample_size
        d.idx[r] = o.data_ptr()
        m = None if masks is None else masks[r]
        if m is not None:
            assert m.is_cuda and m.dtype == torch.uint8 and m.is_contiguous() and tuple(m.shape) == (int(h), int(w))
            d.mask[r] = m.data_ptr()
    d.counter = counters.data_ptr()
    d.debug_flags = 1 if general_path else 0     # (tests: the selection path that is exact for ANY key distribution)
    if n_out is not None:
        assert n_out.dtype == torch.int32 and n_out.numel() >= R and n_out.is_cuda
        d.n_out = n_out.data_ptr()
    return d


def index_draw_weighted(h: int, w: int, sample_size: int, seed: int, counters: torch.Tensor, out_idx, levels, masks=None,
                        n_out=None, stride=None, general_path: bool = False) -> None:
    """One launch of strotss_index_draw_weighted (csrc/draw.hip): index_draw with importance levels.
    levels: per region a (h, w) uint16 device tensor at THIS scale (65535 = always accepted, 0 = only where nothing else is
    left) or None (that region draws as index_draw does).  nn/strotss_utils.py:make_indices_weighted_np on
    rand.PhiloxStream(seed, t) is the host twin of draw number t."""
    d = _draw_t(h, w, sample_size, seed, counters, out_idx, masks, n_out, stride, general_path)
    assert len(levels) == len(out_idx)
    lv = _hip.DrawLevelsT()
    for r, q in enumerate(levels):
        if q is not None:
            assert q.is_cuda and q.dtype == torch.uint16 and q.is_contiguous() and tuple(q.shape) == (int(h), int(w))
            lv.level[r] = q.data_ptr()
    check(_hip.lib().strotss_index_draw_weighted(C.byref(d), C.byref(lv), stream_ptr()), "index_draw_weighted")


def index_draw_counts(h: int, w: int, masks=None):
    """(max candidates of the grid, min over all offset pairs and regions of the number of candidates that survive the
    mask): what decides whether a scale can draw on the device with a fixed sample count.  masks: boolean (h, w) host arrays
    or None.  Pure host arithmetic."""
    import numpy as np
    from .strotss_utils import sampling_steps
    sx, sy = sampling_steps(int(h), int(w))
    most = -(-h // sx) * -(-w // sy)
    least = None
    for ox in range(sx):
        for oy in range(sy):
            if masks is None or all(m is None for m in masks):
                cnt = len(range(ox, h, sx)) * len(range(oy, w, sy))
            else:
                cnt = min(int(np.asarray(m)[ox::sx, oy::sy].sum()) if m is not None else
                          len(range(ox, h, sx)) * len(range(oy, w, sy)) for m in masks)
            least = cnt if least is None else min(least, cnt)
    return most, least


class Workspaces:
    """The scratch memory of one owner: the C ABI never allocates.  Whatever a captured hipGraph points into belongs to the
    object that owns the graph -- a StepEngine and its trunk draw from an instance of their own -- so it is released with
    that object and, once frozen, cannot be reallocated under the graph.  The module-level `workspaces` serves every caller
    that passes no `ws`: one-off operators, feature extraction, the mask and colour tools."""

    def __init__(self):
        self.bufs = {}                   # (tag, device) -> grow-only scratch
        self.fixed = {}                  # (tag, device, key) -> zeroed buffer of one layout
        self.selfsim_record = None       # what the "selfsim" buffer holds (selfsim_fwd_bwd; _pred_panels_after_selfsim)
        self.frozen = False

    def get(self, tag: str, nbytes: int, device) -> torch.Tensor:
        """grow-only scratch of at least `nbytes` (and 256) per (tag, device); growth REALLOCATES, which a captured graph
        must never see (it holds the old pointer): after freeze() it is an error"""
        key = (tag, str(device))
        b = self.bufs.get(key)
        if b is None or b.numel() < nbytes:
            if b is not None and self.frozen:
                raise _hip.StrotssHipError(f"workspace {tag!r} is frozen under a captured graph at {b.numel()} bytes and "
                                           f"cannot grow to {nbytes}")
            b = torch.empty(max(nbytes, 256), dtype=torch.uint8, device=device)
            self.bufs[key] = b
        return b

    def zeroed(self, tag: str, key, nbytes: int, device) -> torch.Tensor:
        """the zero-initialised buffer of (tag, device, key), `key` the caller's shape key: never shared between shapes and
        never grown.  A ticketed reduction leaves its counter at zero but its partials dirty, so only a buffer that is used
        with one fixed layout stays valid from call to call."""
        key = (tag, str(device), key)
        b = self.fixed.get(key)
        if b is None:
            b = self.fixed[key] = _zeroed_workspace(nbytes, device)
        return b

    def freeze(self) -> None:
        """from now on a `get` that would have to grow a buffer raises; one that fits, and a new tag, are served as before"""
        self.frozen = True


workspaces = Workspaces()


def row_inv_norm(x: torch.Tensor, n: int) -> torch.Tensor:
    require(x, "features")
    r = torch.zeros(x.shape[0], dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_row_inv_norm(ptr(x), n, x.shape[1], ptr(r), stream_ptr()), "row_inv_norm")
    return r


# ------------------------------------------------------------------ region clustering
def _kmeans_rows(x: torch.Tensor, inv_norm: torch.Tensor, n: int, d: int, centres: torch.Tensor, k: int) -> int:
    """checks of the two k-means wrappers -> ld"""
    require(x, "feature rows")
    require(inv_norm, "inverse norms")
    require(centres, "centres")
    ld = int(x.shape[1])
    if not (x.dim() == 2 and 0 < n <= int(x.shape[0]) and 0 < d <= ld and inv_norm.numel() >= n):
        raise ValueError(f"{n} rows of {d} columns in a feature buffer of shape {tuple(x.shape)} with {inv_norm.numel()} norms")
    if not 1 <= k <= _hip.KMEANS_MAX_K or centres.dim() != 2 or int(centres.shape[0]) < k or int(centres.shape[1]) != ld:
        raise ValueError(f"{k} centres in a buffer of shape {tuple(centres.shape)}: expected 1..{_hip.KMEANS_MAX_K} rows of {ld}")
    return ld


def kmeans_assign(x: torch.Tensor, inv_norm: torch.Tensor, n: int, d: int, centres: torch.Tensor, k: int):
    """(label, best, second) of strotss_kmeans_assign: per row i < n of the zero-padded (rows, ld) buffer x the first arg-max j
    of (x_i . centres_j) inv_norm_i (int32), that value and the largest of the others (-inf for k == 1); three (n,) tensors."""
    ld = _kmeans_rows(x, inv_norm, n, d, centres, k)
    label = torch.empty(n, dtype=torch.int32, device=x.device)
    best = torch.empty(n, dtype=torch.float32, device=x.device)
    second = torch.empty(n, dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_kmeans_assign(ptr(x), ptr(inv_norm), n, d, ld, ptr(centres), k, ptr(label), ptr(best), ptr(second),
                                           stream_ptr()), "kmeans_assign")
    return label, best, second


def kmeans_update(x: torch.Tensor, inv_norm: torch.Tensor, label: torch.Tensor, n: int, d: int, k: int,
                  centres: torch.Tensor, ws: Optional["Workspaces"] = None) -> torch.Tensor:
    """strotss_kmeans_update: centres[j] <- the normalised float64 sum of the unit rows with label j, in place (an empty
    cluster keeps its centre); -> count (k,) int32.  label: (>= n,) int32; values outside 0..k-1 are skipped."""
    ld = _kmeans_rows(x, inv_norm, n, d, centres, k)
    if not (label.is_cuda and label.dtype == torch.int32 and label.is_contiguous() and label.numel() >= n):
        raise _hip.StrotssHipError(f"labels must be a contiguous int32 CUDA/HIP tensor of >= {n} values")
    lib = _hip.lib()
    nb = int(lib.strotss_kmeans_update_workspace_bytes(n, ld, k))
    if nb == 0:
        raise _hip.StrotssHipError(f"kmeans_update: bad sizes n {n}, ld {ld}, k {k}")
    buf = (ws or workspaces).get("kmeans", nb, x.device)
    count = torch.empty(k, dtype=torch.int32, device=x.device)
    check(lib.strotss_kmeans_update(ptr(x), ptr(inv_norm), ptr(label), n, d, ld, k, ptr(centres), ptr(count), ptr(buf), nb,
                                    stream_ptr()), "kmeans_update")
    return count


# ------------------------------------------------------------------ mask refinement
def refine_labels(img: torch.Tensor, grid: torch.Tensor, k: int, radius: int, sigma_s: float, sigma_r: float,
                  votes: bool = False, means: bool = False, ws: Optional["Workspaces"] = None):
    """strotss_refine_labels: the (gh, gw) int32 label grid of an (h, w, 3) image brought to (h, w) by a joint bilateral vote
    among the (2 radius + 1)^2 cells around each pixel's own.  -> (label (h, w) int32, count (k,) int32, best, second, mean):
    best / second (h, w) float64 with votes=True, mean the (gh, gw, 3) float32 cell colours with means=True, else None.  Two
    launches on the current stream; the library refuses gh > h, gw > w, k outside 1..16, a radius outside 1..4, a sigma <= 0."""
    h, w = _rgb_image(img, "image")
    if not (grid.is_cuda and grid.dtype == torch.int32 and grid.is_contiguous() and grid.dim() == 2):
        raise _hip.StrotssHipError("the label grid must be a contiguous (gh, gw) int32 CUDA/HIP tensor")
    gh, gw = int(grid.shape[0]), int(grid.shape[1])
    lib = _hip.lib()
    nb = int(lib.strotss_refine_labels_workspace_bytes(h, w, gh, gw))
    if nb == 0:
        raise ValueError(f"refine_labels: a {gh} x {gw} label grid for an image of {h} x {w} (the grid may not be larger)")
    buf = (ws or workspaces).get("refine", nb, img.device)
    label = torch.empty((h, w), dtype=torch.int32, device=img.device)
    count = torch.empty(int(k), dtype=torch.int32, device=img.device) if 1 <= int(k) <= _hip.KMEANS_MAX_K else None
    best = torch.empty((h, w), dtype=torch.float64, device=img.device) if votes else None
    second = torch.empty((h, w), dtype=torch.float64, device=img.device) if votes else None
    check(lib.strotss_refine_labels(ptr(img), h, w, ptr(grid), gh, gw, int(k), int(radius), float(sigma_s), float(sigma_r),
                                    ptr(label), ptr(best), ptr(second), ptr(count), ptr(buf), nb, stream_ptr()), "refine_labels")
    mean = buf[:gh * gw * 12].view(torch.float32).reshape(gh, gw, 3).clone() if means else None
    return label, count, best, second, mean


# ------------------------------------------------------------------ region tracking
def _int32_on_device(t: torch.Tensor, n: int, name: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= n):
        raise _hip.StrotssHipError(f"{name} must be a contiguous int32 CUDA/HIP tensor of >= {n} values")
    return t


def label_warp(prev_grid: torch.Tensor, k: int, flow: torch.Tensor, certainty: Optional[torch.Tensor] = None) -> torch.Tensor:
    """strotss_label_warp: the (gh, gw) int32 prior labels of a frame from the (gh, gw) int32 label grid of an earlier one,
    along the backward flow (h, w, 2) = (dx, dy) between the two; -1 where the flow is not finite, leaves the image, the
    certainty (h, w) at the cell's probe pixel is below 0.5 (None: no test) or the label found lies outside 0..k-1.  One
    launch on the current stream; the library refuses gh > h, gw > w and k outside 1..16."""
    if prev_grid.dim() != 2:
        raise _hip.StrotssHipError("the label grid must be a contiguous (gh, gw) int32 CUDA/HIP tensor")
    gh, gw = int(prev_grid.shape[0]), int(prev_grid.shape[1])
    _int32_on_device(prev_grid, gh * gw, "the label grid")
    require(flow, "backward flow")
    if flow.dim() != 3 or int(flow.shape[2]) != 2:
        raise ValueError(f"a flow of shape {tuple(flow.shape)}: expected (h, w, 2)")
    h, w = int(flow.shape[0]), int(flow.shape[1])
    if certainty is not None:
        require(certainty, "certainty")
        if certainty.numel() != h * w:
            raise ValueError(f"a certainty of shape {tuple(certainty.shape)} for a flow of {h} x {w}")
    prior = torch.empty((gh, gw), dtype=torch.int32, device=flow.device)
    check(_hip.lib().strotss_label_warp(ptr(prev_grid), gh, gw, int(k), ptr(flow), ptr(certainty), h, w, ptr(prior),
                                        stream_ptr()), "label_warp")
    return prior


def kmeans_assign_prior(x: torch.Tensor, inv_norm: torch.Tensor, n: int, d: int, centres: torch.Tensor, k: int,
                        prior: torch.Tensor, beta: float):
    """(label, best, second) of strotss_kmeans_assign_prior: kmeans_assign with beta added to the score of each row's prior
    label (int32, (>= n,); a value outside 0..k-1 adds nothing); best and second are raw scores.  The library refuses a beta
    that is not finite or outside [0, 2]."""
    ld = _kmeans_rows(x, inv_norm, n, d, centres, k)
    _int32_on_device(prior, n, "the prior labels")
    label = torch.empty(n, dtype=torch.int32, device=x.device)
    best = torch.empty(n, dtype=torch.float32, device=x.device)
    second = torch.empty(n, dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_kmeans_assign_prior(ptr(x), ptr(inv_norm), n, d, ld, ptr(centres), k, ptr(prior), float(beta),
                                                 ptr(label), ptr(best), ptr(second), stream_ptr()), "kmeans_assign_prior")
    return label, best, second


# ------------------------------------------------------------------ scribble masks
def kmeans_scores(x: torch.Tensor, inv_norm: torch.Tensor, n: int, d: int, centres: torch.Tensor, k: int) -> torch.Tensor:
    """strotss_kmeans_scores: the (n, k) float32 scores (x_i . centres_j) inv_norm_i, the bits kmeans_assign compares"""
    ld = _kmeans_rows(x, inv_norm, n, d, centres, k)
    scores = torch.empty((n, k), dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_kmeans_scores(ptr(x), ptr(inv_norm), n, d, ld, ptr(centres), k, ptr(scores), stream_ptr()),
          "kmeans_scores")
    return scores


def scribble_labels(img: torch.Tensor, stroke: torch.Tensor, scores: torch.Tensor, tau: float, lam: float, sigma: float,
                    iters: int, iters_per_launch: int = 0, planes: bool = False, ws: Optional["Workspaces"] = None,
                    out=None):
    """strotss_scribble_labels: the strokes of an (h, w, 3) image -- stroke (h, w) int32, a label 0..k-1 or anything else --
    spread over the image by `iters` Jacobi sweeps of a screened random walker whose unary is the softmax at temperature tau of
    the bilinearly sampled (gh, gw, k) score grid.  -> (label (h, w) int32, count (k,) int32, x): x the (k, h, w) float32
    planes after the last sweep with planes=True, else None.  iters_per_launch: 0 (the library's choice), 1, 2, 4 or 8; the
    same bits for each.  out: None, or (label, count, x) to write into (x None without planes).  The library refuses k outside 2..7, a tau, lambda or sigma <= 0 and iters outside 1..1024."""
    h, w = _rgb_image(img, "image")
    _int32_on_device(stroke, h * w, "the stroke labels")
    require(scores, "score grid")
    if scores.dim() != 3 or tuple(stroke.shape) != (h, w):
        raise ValueError(f"a score grid of shape {tuple(scores.shape)} and strokes of shape {tuple(stroke.shape)} for an image "
                         f"of {h} x {w}: expected (gh, gw, k) and (h, w)")
    gh, gw, k = (int(v) for v in scores.shape)
    lib = _hip.lib()
    nb = int(lib.strotss_scribble_workspace_bytes(h, w, k))
    if nb == 0:
        raise ValueError(f"scribble_labels: {k} regions on an image of {h} x {w} (expected 2..{_hip.SCRIBBLE_MAX_K} regions)")
    buf = (ws or workspaces).get("scribble", nb, img.device)
    if out is None:
        label = torch.empty((h, w), dtype=torch.int32, device=img.device)
        count = torch.empty(k, dtype=torch.int32, device=img.device)
        x = torch.empty((k, h, w), dtype=torch.float32, device=img.device) if planes else None
    else:
        label, count, x = out
        _int32_on_device(label, h * w, "the labels")
        _int32_on_device(count, k, "the region counts")
        assert (x is not None) == bool(planes)
        if planes:
            require(x, "the planes")
            assert x.numel() == k * h * w
    check(lib.strotss_scribble_labels(ptr(img), ptr(stroke), h, w, ptr(scores), gh, gw, k, float(tau), float(lam), float(sigma),
                                      int(iters), int(iters_per_launch), ptr(label), ptr(count), ptr(x), ptr(buf), nb,
                                      stream_ptr()), "scribble_labels")
    return label, count, x


def cosine_distance(x, rx, nx, y, ry, ny) -> torch.Tensor:
    ldc = pad32(ny)
    Cm = torch.empty((nx, ldc), dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_cosine_distance(ptr(x), ptr(rx), nx, ptr(y), ptr(ry), ny, x.shape[1], ptr(Cm),
                                             ldc, stream_ptr()), "cosine_distance")
    return Cm


def l2_distance(x, nx, y, ny, d) -> torch.Tensor:
    """sqrt(max(|x_i|^2 + |y_j|^2 - 2 x_i.y_j, 1e-6) / d) on the f32 MFMA; x, y: zero-padded (rows, ld) buffers."""
    ldc = pad32(ny)
    Cm = torch.empty((nx, ldc), dtype=torch.float32, device=x.device)
    ws = torch.empty(nx + ny, dtype=torch.float32, device=x.device)
    check(_hip.lib().strotss_l2_distance(ptr(x), nx, ptr(y), ny, d, x.shape[1], ptr(Cm), ldc, ptr(ws), stream_ptr()),
          "l2_distance")
    return Cm


def row_inv_norm_x3(x, n):
    """(r, panels): the row norms' reciprocals and the rows as x3 panels (three bf16 planes per value) for
    cosine_distance_x3."""
    require(x, "feature matrix")
    r = torch.empty(pad32(n), dtype=torch.float32, device=x.device)
    panels = torch.empty(3 * n * x.shape[1], dtype=torch.bfloat16, device=x.device)
    check(_hip.lib().strotss_row_inv_norm_x3(ptr(x), n, x.shape[1], ptr(r), ptr(panels), stream_ptr()), "row_inv_norm_x3")
    return r, panels


def cosine_distance_x3(xp, rx, nx, yp, ry, ny, ld) -> torch.Tensor:
    """cosine_distance on the bf16x3 GEMM core from the x3 panels of x and y (row_inv_norm_x3)."""
    ldc = pad32(ny)
    Cm = torch.empty((nx, ldc), dtype=torch.float32, device=rx.device)
    check(_hip.lib().strotss_cosine_distance_x3(ptr(xp), ptr(rx), nx, ptr(yp), ptr(ry), ny, ld, ptr(Cm), ldc,
                                                stream_ptr()), "cosine_distance_x3")
    return Cm


def selfsim_fwd_bwd(pred, content, n, d, gscale, gpred, loss_out, ws=None):
    l = _hip.lib()
    nb = l.strotss_selfsim_workspace_bytes(n, pred.shape[1])
    buf = (ws or workspaces).get("selfsim", nb, pred.device)
    check(l.strotss_selfsim_fwd_bwd(ptr(pred), ptr(content), n, d, pred.shape[1], gscale, ptr(gpred),
                                    ptr(loss_out), ptr(buf), nb, stream_ptr()), "selfsim_fwd_bwd")
    _record_selfsim(ws, buf, nb, pred, n)


def selfsim_weighted_fwd_bwd(pred, content, col_weight, n, d, gscale, gpred, loss_out, ws=None):
    """selfsim_fwd_bwd with the content term weighted per sampled column (strotss_selfsim_weighted_fwd_bwd): col_weight is a
    float32 device vector of >= n values, finite and >= 0 (None: selfsim_fwd_bwd itself).  Same workspace, same record: the
    relaxed EMD borrows the prediction rows' norms and panels from it as after the unweighted call."""
    if col_weight is None:
        return selfsim_fwd_bwd(pred, content, n, d, gscale, gpred, loss_out, ws=ws)
    require(col_weight, "column weights")
    assert col_weight.numel() >= n
    l = _hip.lib()
    nb = l.strotss_selfsim_workspace_bytes(n, pred.shape[1])
    buf = (ws or workspaces).get("selfsim", nb, pred.device)
    check(l.strotss_selfsim_weighted_fwd_bwd(ptr(pred), ptr(content), ptr(col_weight), n, d, pred.shape[1], gscale, ptr(gpred),
                                             ptr(loss_out), ptr(buf), nb, stream_ptr()), "selfsim_weighted_fwd_bwd")
    _record_selfsim(ws, buf, nb, pred, n)


def _record_selfsim(ws, buf, nb, pred, n) -> None:
    # what the selfsim buffer of `ws` now holds (reciprocal norms + x3 panels of exactly these prediction rows), for the borrower
    (ws or workspaces).selfsim_record = (buf.data_ptr(), nb, ptr(pred), n, int(pred.shape[1]), stream_ptr())


remd_borrow_stats = {"borrowed": 0, "plain": 0}      # which path remd_cos_fwd_bwd_after_selfsim took (tests read it)


def remd_cos_fwd_bwd(style, rs, ns, pred, n, d, gscale, gpred, loss_out, swapped=False, ws=None):
    """swapped: `pred` is the reference's FIRST argument (gradient to the target side; STROTSS_REMD_SWAPPED)"""
    l = _hip.lib()
    nb = l.strotss_remd_workspace_bytes(ns, n, pred.shape[1])
    buf = (ws or workspaces).get("remd", nb, pred.device)
    check(l.strotss_remd_cos_fwd_bwd(ptr(style), ptr(rs), ns, ptr(pred), n, d, pred.shape[1], gscale,
                                     ptr(gpred), ptr(loss_out), int(swapped), ptr(buf), nb, stream_ptr()), "remd_cos_fwd_bwd")


def _pred_panels_after_selfsim(pred, n, style_panels, ws=None):
    """What selfsim_fwd_bwd is KNOWN to have left in its workspace for exactly these prediction rows: (reciprocal norms,
    prediction panels, style panels) as pointers, or None where the record that call leaves on `ws` does not match -- other
    rows, a regrown or re-used buffer, another count or stride, another stream.  The panels come as a pair: both are None
    where the library hands out none (the cost matrices on the f32 MFMA, STROTSS_X3=0) or the StyleTarget has none."""
    l = _hip.lib()
    ld = int(pred.shape[1])
    nb = l.strotss_selfsim_workspace_bytes(n, ld)
    ws = ws or workspaces
    buf = ws.get("selfsim", nb, pred.device)
    if ws.selfsim_record != (buf.data_ptr(), nb, ptr(pred), n, ld, stream_ptr()):
        return None
    rp, xp = C.c_void_p(), C.c_void_p()
    check(l.strotss_selfsim_pred_panels(ptr(buf), nb, n, ld, C.byref(rp), C.byref(xp)), "selfsim_pred_panels")
    both = style_panels is not None and bool(xp.value)
    return rp.value, xp.value if both else None, ptr(style_panels) if both else None


def _pred_panels_or_raise(who, pred, n, style_panels, ws=None):
    """_pred_panels_after_selfsim for the terms that have no plain call to fall back to: a mismatch is an error"""
    got = _pred_panels_after_selfsim(pred, n, style_panels, ws)
    if got is None:
        raise _hip.StrotssHipError(f"{who}: selfsim_fwd_bwd has not just run on these rows")
    return got


def remd_cos_fwd_bwd_after_selfsim(style, rs, style_panels, ns, pred, n, d, gscale, gpred, loss_out, ws=None):
    """remd_cos_fwd_bwd for the prediction rows that selfsim_fwd_bwd has just processed (_pred_panels_after_selfsim; a
    mismatch falls back to the plain call, which makes its own norms and panels): their reciprocal norms and x3 panels are
    taken from that workspace, the style rows' panels from `style_panels` (row_inv_norm_x3(style)[1], constant within a
    scale) -- bit for bit remd_cos_fwd_bwd, one launch and two passes over the rows less.  No pair of panels: the plain call."""
    got = _pred_panels_after_selfsim(pred, n, style_panels, ws)
    if got is None or got[1] is None:
        remd_borrow_stats["plain"] += 1
        return remd_cos_fwd_bwd(style, rs, ns, pred, n, d, gscale, gpred, loss_out, ws=ws)
    rp, xp, sp = got
    remd_borrow_stats["borrowed"] += 1
    l = _hip.lib()
    ld = pred.shape[1]
    nbr = l.strotss_remd_workspace_bytes(ns, n, ld)
    wsr = (ws or workspaces).get("remd", nbr, pred.device)
    check(l.strotss_remd_cos_fwd_bwd_panels(ptr(style), ptr(rs), sp, ns, ptr(pred), rp, xp, n, d, ld,
                                            gscale, ptr(gpred), ptr(loss_out), ptr(wsr), nbr, stream_ptr()),
          "remd_cos_fwd_bwd_panels")


def step_losses_available() -> bool:
    """the library's grouped loss entries would not refuse on account of its switches (strotss_step_losses_available), and
    the host-only STROTSS_GROUPED_LOSSES does not switch them off"""
    return bool(_hip.load_library().strotss_step_losses_available()) and env_int("STROTSS_GROUPED_LOSSES", 1) != 0


def step_losses_fwd_bwd(pred, content, n, d, style, rs, style_panels, ns, style_mean, style_cov, g_content, g_moment, g_remd,
                        g_palette, gpred, loss_content, loss_moment, loss_remd, loss_palette, ws=None):
    """self_similarity + moment_matching + relaxed_emd (cosine) + the YUV palette relaxed_emd of one train step in ONE call
    (strotss_step_losses_fwd_bwd): one prologue launch, the three forward GEMMs in one launch, 13 launches in all; bit for
    bit selfsim_fwd_bwd, moment_fwd_bwd, remd_cos_fwd_bwd_after_selfsim, palette_remd_fwd_bwd in this order."""
    l = _hip.lib()
    ld = int(pred.shape[1])
    nb = l.strotss_step_losses_workspace_bytes(ns, n, ld)
    buf = (ws or workspaces).get("step_losses", nb, pred.device)
    check(l.strotss_step_losses_fwd_bwd(ptr(pred), ptr(content), n, d, ld, ptr(style), ptr(rs), ptr(style_panels), ns,
                                        ptr(style_mean), ptr(style_cov), float(g_content), float(g_moment), float(g_remd),
                                        float(g_palette), ptr(gpred), ptr(loss_content), ptr(loss_moment), ptr(loss_remd),
                                        ptr(loss_palette), ptr(buf), nb, stream_ptr()), "step_losses_fwd_bwd")


def make_style_set(targets, weights) -> "_hip.StyleSetT":
    """strotss_style_set_t of StyleTargets (feats, inv_norm, panels, ns, mean, cov) and their weights"""
    if not 1 <= len(targets) <= _hip.MAX_STYLES or len(weights) != len(targets):
        raise ValueError(f"a style set holds 1..{_hip.MAX_STYLES} targets with one weight each")
    s = _hip.StyleSetT()
    s.n_styles = len(targets)
    for k, (t, w) in enumerate(zip(targets, weights)):
        if t.panels is None:
            raise _hip.StrotssHipError("blended step: every style target needs its x3 panels (ld % 32 == 0)")
        s.feats[k], s.inv_norm[k], s.panels[k] = ptr(t.feats), ptr(t.inv_norm), ptr(t.panels)
        s.ns[k], s.mean[k], s.cov[k], s.weight[k] = int(t.ns), ptr(t.mean), ptr(t.cov), float(w)
    return s


def step_losses_blend_fwd_bwd(pred, content, n, d, style_set, g_content, g_moment, g_remd, g_palette, gpred, loss_content,
                              loss_moment, loss_remd, loss_palette, ws=None):
    """The four loss terms against a weighted style set (make_style_set) in ONE call (strotss_step_losses_blend_fwd_bwd):
    the launch count of step_losses_fwd_bwd whatever the number of styles.  loss_moment / loss_remd / loss_palette receive
    one UNWEIGHTED value per style; gpred += g_content dLc + sum_k w_k (g_moment dLm_k + g_remd dLr_k + g_palette dLp_k)."""
    l = _hip.lib()
    ld = int(pred.shape[1])
    nb = l.strotss_step_losses_blend_workspace_bytes(C.byref(style_set), n, ld)
    if nb == 0:
        raise _hip.StrotssHipError("step_losses_blend: invalid style set")
    buf = (ws or workspaces).get("step_losses_blend", nb, pred.device)
    check(l.strotss_step_losses_blend_fwd_bwd(ptr(pred), ptr(content), n, d, ld, C.byref(style_set), float(g_content),
                                              float(g_moment), float(g_remd), float(g_palette), ptr(gpred), ptr(loss_content),
                                              ptr(loss_moment), ptr(loss_remd), ptr(loss_palette), ptr(buf), nb, stream_ptr()),
          "step_losses_blend_fwd_bwd")


def step_losses_cw_fwd_bwd(pred, content, n, d, col_weight, style_set, g_content, g_moment, g_remd, g_palette, gpred,
                           loss_content, loss_moment, loss_remd, loss_palette, ws=None):
    """step_losses_blend_fwd_bwd (any number of styles, one included) with the content term weighted per sampled column
    (strotss_step_losses_cw_fwd_bwd; col_weight: float32 device vector of >= n values, finite and >= 0, or None: the
    unweighted term).  One style: the single-style launches (of weight 1: bit for bit step_losses_fwd_bwd); several: the
    blended ones."""
    if col_weight is not None:
        require(col_weight, "column weights")
        assert col_weight.numel() >= n
    l = _hip.lib()
    ld = int(pred.shape[1])
    nb = l.strotss_step_losses_blend_workspace_bytes(C.byref(style_set), n, ld)
    if nb == 0:
        raise _hip.StrotssHipError("step_losses_cw: invalid style set")
    buf = (ws or workspaces).get("step_losses_blend", nb, pred.device)
    check(l.strotss_step_losses_cw_fwd_bwd(ptr(pred), ptr(content), n, d, ld, ptr(col_weight), C.byref(style_set),
                                           float(g_content), float(g_moment), float(g_remd), float(g_palette), ptr(gpred),
                                           ptr(loss_content), ptr(loss_moment), ptr(loss_remd), ptr(loss_palette), ptr(buf), nb,
                                           stream_ptr()), "step_losses_cw_fwd_bwd")


def sinkhorn_cos_fwd_bwd(style, rs, ns, pred, n, d, l, n_iter, gscale, gpred, loss_out, ws=None):
    lib = _hip.lib()
    nb = lib.strotss_sinkhorn_workspace_bytes(ns, n, n_iter)
    buf = (ws or workspaces).get("sinkhorn", nb, pred.device)
    check(lib.strotss_sinkhorn_cos_fwd_bwd(ptr(style), ptr(rs), ns, ptr(pred), n, d, pred.shape[1], float(l), int(n_iter),
                                           gscale, ptr(gpred), ptr(loss_out), ptr(buf), nb, stream_ptr()),
          "sinkhorn_cos_fwd_bwd")


def sinkhorn_cos_fwd_bwd_after_selfsim(style, rs, style_panels, ns, pred, n, d, l, n_iter, gscale, gpred, loss_out, ws=None):
    """The step's Sinkhorn term (strotss_sinkhorn_cos_fwd_bwd_panels) for the prediction rows that
    selfsim_fwd_bwd has just processed: their reciprocal norms and x3 panels come from that call's workspace, the style rows'
    panels from `style_panels` (_pred_panels_after_selfsim: both panels or neither).  Unlike the relaxed EMD there is no plain
    call to fall back to: rows other than those the content loss left its record for are an error."""
    l_ = _hip.lib()
    ld = pred.shape[1]
    rp, xp, sp = _pred_panels_or_raise("sinkhorn_cos_fwd_bwd_after_selfsim", pred, n, style_panels, ws)
    nbs = l_.strotss_sinkhorn_step_workspace_bytes(ns, n, int(n_iter))
    wss = (ws or workspaces).get("sinkhorn_step", nbs, pred.device)
    check(l_.strotss_sinkhorn_cos_fwd_bwd_panels(ptr(style), ptr(rs), sp, ns, ptr(pred), rp, xp, n, d, ld, float(l),
                                                 int(n_iter), float(gscale), ptr(gpred), ptr(loss_out), ptr(wss), nbs,
                                                 stream_ptr()),
          "sinkhorn_cos_fwd_bwd_panels")


def sinkhorn_log_cos_fwd_bwd_after_selfsim(style, rs, style_panels, ns, pred, n, d, l, n_iter, gscale, gpred, loss_out, ws=None):
    """The step's Sinkhorn term in the log domain (strotss_sinkhorn_log_cos_fwd_bwd_panels), called as
    sinkhorn_cos_fwd_bwd_after_selfsim is: the prediction rows' norms and x3 panels from the content loss's workspace, both
    panels or neither, and rows other than those the content loss left its record for an error."""
    l_ = _hip.lib()
    ld = pred.shape[1]
    rp, xp, sp = _pred_panels_or_raise("sinkhorn_log_cos_fwd_bwd_after_selfsim", pred, n, style_panels, ws)
    nbs = l_.strotss_sinkhorn_log_step_workspace_bytes(ns, n, int(n_iter))
    if nbs == 0:
        raise _hip.StrotssHipError(f"sinkhorn_log_cos_fwd_bwd_after_selfsim: invalid sizes ns={ns} n={n} n_iter={n_iter}")
    wss = (ws or workspaces).get("sinkhorn_log_step", nbs, pred.device)
    check(l_.strotss_sinkhorn_log_cos_fwd_bwd_panels(ptr(style), ptr(rs), sp, ns, ptr(pred), rp, xp, n, d, ld, float(l),
                                                     int(n_iter), float(gscale), ptr(gpred), ptr(loss_out), ptr(wss), nbs,
                                                     stream_ptr()),
          "sinkhorn_log_cos_fwd_bwd_panels")


def sliced_cos_fwd_bwd_after_selfsim(style, rs, style_panels, ns, pred, n, d, n_proj, seed, counter, gscale, gpred, loss_out,
                                     ws=None):
    """The step's sliced Wasserstein term (strotss_sliced_cos_fwd_bwd) for the prediction rows that
    selfsim_fwd_bwd has just processed: their reciprocal norms and x3 panels come from that call's workspace, the style rows'
    panels from `style_panels` (_pred_panels_after_selfsim: both panels or neither).  `counter`: one int32 on the device, the
    draw number of the directions; the call leaves it one higher.  As for the Sinkhorn term, rows other than those the
    content loss left its record for are an error."""
    l_ = _hip.lib()
    ld = pred.shape[1]
    assert counter.dtype == torch.int32 and counter.numel() >= 1 and counter.is_cuda
    rp, xp, sp = _pred_panels_or_raise("sliced_cos_fwd_bwd_after_selfsim", pred, n, style_panels, ws)
    nbs = l_.strotss_sliced_workspace_bytes(ns, n, ld, int(n_proj))
    wss = (ws or workspaces).get("sliced_step", nbs, pred.device)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    check(l_.strotss_sliced_cos_fwd_bwd(ptr(style), ptr(rs), sp, ns, ptr(pred), rp, xp, n, d, ld, int(n_proj),
                                        seed & 0xFFFFFFFF, seed >> 32, ptr(counter), float(gscale), ptr(gpred), ptr(loss_out),
                                        ptr(wss), nbs, stream_ptr()),
          "sliced_cos_fwd_bwd")


def sinkhorn_metric_fwd_bwd(style, ns, pred, n, d, metric: str, l, n_iter, gscale, gpred, loss_out, ws=None):
    lib = _hip.lib()
    nb = lib.strotss_sinkhorn_metric_workspace_bytes(ns, n, n_iter)
    buf = (ws or workspaces).get("sinkhorn", nb, pred.device)
    check(lib.strotss_sinkhorn_metric_fwd_bwd(ptr(style), ns, ptr(pred), n, d, pred.shape[1], REMD_METRICS[metric], float(l),
                                              int(n_iter), gscale, ptr(gpred), ptr(loss_out), ptr(buf), nb, stream_ptr()),
          "sinkhorn_metric_fwd_bwd")


def palette_remd_fwd_bwd(style, ns, pred, n, gscale, gpred, loss_out, rgb_to_yuv=True, swapped=False, ws=None):
    l = _hip.lib()
    nb = l.strotss_remd_workspace_bytes(ns, n, 0)
    buf = (ws or workspaces).get("remd", nb, pred.device)
    assert style.shape[1] == pred.shape[1]
    check(l.strotss_palette_remd_fwd_bwd(ptr(style), ns, ptr(pred), n, pred.shape[1], int(rgb_to_yuv), gscale,
                                         ptr(gpred), ptr(loss_out), int(swapped), ptr(buf), nb, stream_ptr()), "palette_remd_fwd_bwd")


def palette_sliced_fwd_bwd(style, ns, pred, n, dirs, gscale, gpred, loss_out, rgb_to_yuv=True, ws=None):
    """The sliced palette term (strotss_palette_sliced_fwd_bwd) where palette_remd_fwd_bwd stands:
    dirs an (n_proj, 3) float32 device tensor of unit directions (rand.palette_directions)"""
    l = _hip.lib()
    assert style.shape[1] == pred.shape[1] and dirs.dtype == torch.float32 and dirs.is_contiguous() and dirs.shape[1] == 3
    n_proj = int(dirs.shape[0])
    nb = l.strotss_palette_sliced_workspace_bytes(ns, n, n_proj)
    buf = (ws or workspaces).get("palette_sliced", nb, pred.device)
    check(l.strotss_palette_sliced_fwd_bwd(ptr(style), ns, ptr(pred), n, pred.shape[1], int(rgb_to_yuv), ptr(dirs), n_proj,
                                           gscale, ptr(gpred), ptr(loss_out), ptr(buf), nb, stream_ptr()),
          "palette_sliced_fwd_bwd")


REMD_METRICS = {"l2": 1, "both": 2}      # STROTSS_METRIC_L2 / STROTSS_METRIC_BOTH (include/strotss_hip.h)


def remd_metric_fwd_bwd(style, ns, pred, n, d, metric: str, gscale, gpred, loss_out, swapped=False, ws=None):
    """relaxed_emd with dist_metrics 'l2' / 'both' at any width (reference losses.py:18-28, 69-80)."""
    l = _hip.lib()
    nb = l.strotss_remd_metric_workspace_bytes(ns, n)
    buf = (ws or workspaces).get("remd_metric", nb, pred.device)
    assert style.shape[1] == pred.shape[1]
    check(l.strotss_remd_metric_fwd_bwd(ptr(style), ns, ptr(pred), n, d, pred.shape[1], REMD_METRICS[metric], gscale,
                                        ptr(gpred), ptr(loss_out), int(swapped), ptr(buf), nb, stream_ptr()), "remd_metric_fwd_bwd")


def rows_gemm_bwd(W, k, B, x, r, q, n, g, dx):
    """dx[i, :] += g * r[i] * (sum_j W[i, j] B[j, :] - x[i, :] * r[i] * q[i])   for i < n, j < k  (strotss_rows_gemm_bwd):
    the backward of a pairwise distance matrix w.r.t. one of its two row sets (reference losses.py:12-24 under
    tape.gradient) -- W = d(loss)/d(product) scaled by the other side's factors, q = the normalisation's rank-one term.
    The caller zero-fills: the product runs over ALL W.shape[1] columns of W and as many rows of B (k is only validated), so
    columns k .. W.shape[1] - 1 of W must be zero and those rows of B finite for the sum to be the one over j < k."""
    assert W.is_contiguous() and B.is_contiguous() and x.is_contiguous() and dx.is_contiguous()
    assert int(W.shape[1]) % 32 == 0 and int(B.shape[1]) == int(x.shape[1]) == int(dx.shape[1]) and int(B.shape[0]) >= int(W.shape[1])
    check(_hip.lib().strotss_rows_gemm_bwd(ptr(W), int(W.shape[1]), int(k), ptr(B), ptr(x), ptr(r), ptr(q), n, int(x.shape[1]),
                                           float(g), ptr(dx), stream_ptr()), "rows_gemm_bwd")


def moment_stats(x, n, d, ws=None):
    l = _hip.lib()
    ld = x.shape[1]
    nb = l.strotss_moment_workspace_bytes(n, ld)
    buf = (ws or workspaces).get("moment", nb, x.device)
    mean = torch.empty(ld, dtype=torch.float32, device=x.device)
    cov = torch.empty((ld, ld), dtype=torch.float32, device=x.device)
    check(l.strotss_moment_stats(ptr(x), n, d, ld, ptr(mean), ptr(cov), ptr(buf), nb, stream_ptr()),
          "moment_stats")
    return mean, cov


def moment_fwd_bwd(style_mean, style_cov, pred, n, d, gscale, gpred, loss_out, ws=None):
    l = _hip.lib()
    ld = pred.shape[1]
    nb = l.strotss_moment_workspace_bytes(n, ld)
    buf = (ws or workspaces).get("moment", nb, pred.device)
    check(l.strotss_moment_fwd_bwd(ptr(style_mean), ptr(style_cov), ptr(pred), n, d, ld, gscale, ptr(gpred),
                                   ptr(loss_out), ptr(buf), nb, stream_ptr()), "moment_fwd_bwd")


# ------------------------------------------------------------------ optimiser / output
def rmsprop_step(variables, rms, grads, lr: float, rho: float = 0.99, eps: float = 1e-8):
    t = _hip.TensorsT()
    t.n_tensors = len(variables)
    for k, (v, r, g) in enumerate(zip(variables, rms, grads)):
        require(v, "variable"); require(r, "rms"); require(g, "grad")
        assert v.numel() == r.numel() == g.numel()
        t.var[k], t.rms[k], t.grad[k], t.numel[k] = v.data_ptr(), r.data_ptr(), g.data_ptr(), v.numel()
    check(_hip.lib().strotss_rmsprop_step(C.byref(t), lr, rho, eps, stream_ptr()), "rmsprop_step")


def postprocess(img: torch.Tensor) -> torch.Tensor:
    require(img, "image")
    out = torch.empty(img.shape, dtype=torch.uint8, device=img.device)
    ws = torch.empty(2048, dtype=torch.float32, device=img.device)
    check(_hip.lib().strotss_postprocess(ptr(img), img.numel(), ptr(out), ptr(ws), stream_ptr()), "postprocess")
    return out
