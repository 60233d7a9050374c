"""The pixel-space terms of the step: each acts on the folded image between the trunk's pixel gradient (after the all-reduce)
and the fold adjoint, once per step and not averaged over the regions.  A target says what a term is at one scale; a bound
term is a target made ready for one StepEngine.  Its constructor validates, copies what a captured graph reads at replay,
prepares what is made once per scale and takes the scalars and, from `ws` (the engine's Workspaces), the zeroed workspace:
never inside a capture.  run(img, gimg) adds weight * dL/dimg to gimg, img the folded image of this step; report(out) writes
the term's keys into the losses() dict and returns its weighted share of out["loss"]."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np
import torch

from . import _hip, _ops
from .strotss_utils import check_content_weight


def _check_prior_weight(weight, name: str) -> None:
    """ValueError unless `weight` is a real number, not a bool, finite and >= 0"""
    if isinstance(weight, bool) or not isinstance(weight, (int, float, np.integer, np.floating)) or \
            not np.isfinite(weight) or weight < 0:
        raise ValueError(f"{name} must be finite and >= 0, got {weight!r}")


def _check_image(t: torch.Tensor, what: str, h: int, w: int) -> None:
    """ValueError unless `t` is one (h, w, 3) image"""
    if t.numel() != 3 * h * w or tuple(t.shape[-3:]) != (h, w, 3):
        raise ValueError(f"{what} of shape {tuple(t.shape)}: expected ({h}, {w}, 3)")


@dataclass
class TemporalTarget:
    """The temporal term of a frame sequence at one scale: `target` (h, w, 3) the warped previous
    frame, `certainty` (h, w) its certainty, `weight` lambda >= 0.  The step adds
    lambda * L_t = lambda / (3 h w) * sum_p c(p) |x(p) - target(p)|^2 to its loss (strotss_utils.temporal_target_at_scale
    builds the two arrays)."""
    target: torch.Tensor
    certainty: torch.Tensor
    weight: float


@dataclass
class DetailTarget:
    """The Laplacian detail term at one scale: `content` (h, w, 3) or (1, h, w, 3) the content image at
    this scale, `pools` 1..3 distinct pool sizes of {1, 2, 4, 8, 16}, ascending, `weight` >= 0, `cell_map` an optional (h, w)
    map, finite and >= 0, whose pooled values weigh the cells (the content-weight map at this scale).  The step adds
    weight * sum_p L_p, L_p = (1 / (3 hp wp)) sum_k m_p(k) |L (P_p(x) - P_p(content))(k)|^2, to its loss."""
    content: torch.Tensor
    pools: Sequence[int]
    weight: float
    cell_map: Optional[torch.Tensor] = None


@dataclass
class PhotoTarget:
    """The photorealism term at one scale: `content` (h, w, 3) or (1, h, w, 3) the content image at this
    scale (the guide), `radius` 1..4 and `eps` in [1e-4, 1] the windows and the regulariser of its matting Laplacian L,
    `weight` >= 0.  The step adds weight * L_photo, L_photo = (1 / (3 h w)) sum_c x_c^T L x_c, to its loss: the folded image
    may take any colours, but over every window it should be an affine function of the content's."""
    content: torch.Tensor
    radius: int
    eps: float
    weight: float


def check_photo(radius, eps) -> None:
    """ValueError unless radius is an integer in 1..MATTING_MAX_RADIUS and eps finite in [1e-4, 1] (at its float32 value)"""
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 1 <= int(radius) <= _hip.MATTING_MAX_RADIUS:
        raise ValueError(f"photo radius must be an integer in 1..{_hip.MATTING_MAX_RADIUS}, got {radius!r}")
    if isinstance(eps, bool) or not isinstance(eps, (int, float, np.integer, np.floating)) or not np.isfinite(eps) or \
            not np.float32(1e-4) <= np.float32(eps) <= np.float32(1.0):
        raise ValueError(f"photo eps must be finite and in [1e-4, 1], got {eps!r}")


class TemporalTerm:
    """One TemporalTarget or 1..4 of them (long-term targets, DESIGN.md section 13, nearest frame first): ONE launch."""

    def __init__(self, targets: Union[TemporalTarget, Sequence[TemporalTarget]], h: int, w: int, dev, ws: "_ops.Workspaces"):
        terms = [targets] if isinstance(targets, TemporalTarget) else list(targets)
        if not 1 <= len(terms) <= _hip.MAX_TEMPORAL:
            raise ValueError(f"the temporal term takes 1..{_hip.MAX_TEMPORAL} targets, got {len(terms)}")
        for tt in terms:
            if not isinstance(tt, TemporalTarget):
                raise ValueError(f"temporal targets must be TemporalTarget, got {type(tt).__name__}")
            if not np.isfinite(float(tt.weight)) or float(tt.weight) < 0:
                raise ValueError(f"temporal weight must be finite and >= 0, got {tt.weight}")
            _check_image(tt.target, "temporal target", h, w)
            if tt.certainty.numel() != h * w or tuple(tt.certainty.shape[-2:]) != (h, w):
                raise ValueError(f"temporal certainty of shape {tuple(tt.certainty.shape)}: expected ({h}, {w})")
        self.weights = [float(tt.weight) for tt in terms]
        self.targets = [tt.target.float().to(dev).reshape(h, w, 3).contiguous().clone() for tt in terms]
        self.certainties = [tt.certainty.float().to(dev).reshape(h, w).contiguous().clone() for tt in terms]
        self.loss = torch.zeros(len(terms), dtype=torch.float32, device=dev)
        self.workspace = _ops.term_workspace("temporal", h, w, dev, ws, count=len(terms))

    def run(self, img: torch.Tensor, gimg: torch.Tensor) -> None:
        _ops.temporal_multi_fwd_bwd(img, self.targets, self.certainties, self.weights, gimg, self.loss, self.workspace)

    def report(self, out: dict) -> float:
        terms = [float(v) for v in self.loss.tolist()]     # loss_t = sum_j L_j, the share sum_j lambda_j L_j
        out["loss_t"] = float(sum(terms))
        if len(terms) > 1:
            out["loss_t_terms"] = terms
        return sum(lam * lt for lam, lt in zip(self.weights, terms))


class DetailTerm:
    """A DetailTarget: one pooling launch per pool size above 1, one launch per pool size; content and cell map (`cells`: None
    without one) are pooled once, here, by the step's pooling kernel.  Weight 0 runs the term, the gradient bit for bit."""

    def __init__(self, target: DetailTarget, h: int, w: int, dev, ws: "_ops.Workspaces"):
        if not isinstance(target, DetailTarget):
            raise ValueError(f"detail must be a DetailTarget, got {type(target).__name__}")
        self.pools = _ops.check_detail_pools(target.pools)
        _check_prior_weight(target.weight, "detail weight")
        _check_image(target.content, "detail content", h, w)
        self.cells = [None] * len(self.pools)
        if target.cell_map is not None:
            cmap = check_content_weight(target.cell_map, h, w).to(dev).reshape(h, w, 1).contiguous()
            self.cells = [_ops.pool_mean(cmap, p).reshape(_ops.pooled_shape(h, w, p)) for p in self.pools]
        content = target.content.float().to(dev).reshape(h, w, 3).contiguous()
        self.contents = [_ops.pool_mean(content, p) for p in self.pools]
        self.weight, self.gscales = float(target.weight), [float(target.weight)] * len(self.pools)
        self.loss = torch.zeros(len(self.pools), dtype=torch.float32, device=dev)
        self.workspace = _ops.term_workspace("detail", h, w, dev, ws)

    def run(self, img: torch.Tensor, gimg: torch.Tensor) -> None:
        _ops.detail_fwd_bwd(img, self.pools, self.contents, self.cells, self.gscales, gimg, self.loss, self.workspace)

    def report(self, out: dict) -> float:
        terms = [float(v) for v in self.loss.tolist()]
        out["loss_detail"], out["loss_detail_terms"] = float(sum(terms)), terms      # the list always, also for one pool size
        return self.weight * out["loss_detail"]


class TVTerm:
    """The smoothed total variation of the folded image at `weight` > 0 (checked by the engine; 0 is no term): one launch."""

    def __init__(self, weight: float, h: int, w: int, dev, ws: "_ops.Workspaces"):
        self.weight, self.loss = float(weight), torch.zeros(1, dtype=torch.float32, device=dev)
        self.workspace = _ops.term_workspace("tv", h, w, dev, ws)

    def run(self, img: torch.Tensor, gimg: torch.Tensor) -> None:
        _ops.tv_fwd_bwd(img, self.weight, gimg, self.loss, self.workspace)

    def report(self, out: dict) -> float:
        out["loss_tv"] = float(self.loss.item())
        return self.weight * out["loss_tv"]


class PhotoTerm:
    """A PhotoTarget: one launch, the content's window statistics made once, here.  Weight 0: the gradient bit for bit."""

    def __init__(self, target: PhotoTarget, h: int, w: int, dev, ws: "_ops.Workspaces"):
        if not isinstance(target, PhotoTarget):
            raise ValueError(f"photo must be a PhotoTarget, got {type(target).__name__}")
        check_photo(target.radius, target.eps)
        _check_prior_weight(target.weight, "photo weight")
        _check_image(target.content, "photo content", h, w)
        self.weight, self.radius = float(target.weight), int(target.radius)
        self.guide = target.content.float().to(dev).reshape(h, w, 3).contiguous().clone()
        self.stats = _ops.matting_prepare(self.guide, self.radius, float(target.eps))
        self.loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.workspace = _ops.term_workspace("matting", h, w, dev, ws)

    def run(self, img: torch.Tensor, gimg: torch.Tensor) -> None:
        _ops.matting_fwd_bwd(img, self.guide, self.stats, self.radius, self.weight, gimg, self.loss, self.workspace)

    def report(self, out: dict) -> float:
        out["loss_photo"] = float(self.loss.item())
        return self.weight * out["loss_photo"]
