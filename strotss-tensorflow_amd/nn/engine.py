"""The optimisation inner loop of run_strotss.py:104-148 as an explicit, pre-allocated kernel
sequence on one HIP stream (no tracing compiler, no autograd tape):

    fold (5 resize+add)  ->  VGG trunk forward  ->  hypercolumn gather (content, prediction)
    ->  self-similarity / moment / REMD / palette fused forward+backward into one (N, D) gradient
    ->  trunk data-gradient with the taps' scatter-adds interleaved  ->  pixel gradient
    ->  [RCCL all-reduce of the pixel gradient when mask regions are sharded over GPUs]
    ->  fold adjoint (5 transposed resizes)  ->  one multi-tensor RMSprop launch.

Nothing in `step()` synchronises with the host; the three logged scalars stay on the device until
`losses()` is called.  Index sets are inputs (reference: drawn inside the traced train_step,
strotss_utils.py:83-121), so identical index streams give comparable trajectories.
"""
from __future__ import annotations

import gc
import os
from dataclasses import dataclass
from typing import List, Optional, Sequence, Union

import numpy as np
import torch

from . import _hip, _ops, parallel, pixel_terms, rand
from .model import VGGParams, VGGTrunk
from .pixel_terms import DetailTarget, PhotoTarget, TemporalTarget, _check_prior_weight, check_photo     # also for callers
from .strotss_utils import check_content_weight, make_laplacian_pyramid


@dataclass
class StyleTarget:
    """Style side of StyleLoss (run_strotss.py:27-31): sampled once per scale, then constant."""
    feats: torch.Tensor      # (pad32(ns), ld)
    ns: int
    inv_norm: torch.Tensor   # row_inv_norm(feats)
    mean: torch.Tensor       # (ld,)
    cov: torch.Tensor        # (ld, ld)
    panels: Optional[torch.Tensor] = None   # the rows as x3 panels (bf16x3 GEMM operand of the relaxed EMD), made once

    @staticmethod
    def build(feats: torch.Tensor, ns: int, d: int) -> "StyleTarget":
        rs = _ops.row_inv_norm(feats, ns)
        mean, cov = _ops.moment_stats(feats, ns, d)
        panels = _ops.row_inv_norm_x3(feats, ns)[1] if int(feats.shape[1]) % 32 == 0 else None
        return StyleTarget(feats, ns, rs, mean, cov, panels)


def normalise_style_weights(weights: Sequence[float]) -> List[float]:
    """w / sum(w) for 1..MAX_STYLES finite weights >= 0 with a positive sum (ValueError otherwise)"""
    w = [float(x) for x in weights]
    if not 1 <= len(w) <= _hip.MAX_STYLES:
        raise ValueError(f"style blending takes 1..{_hip.MAX_STYLES} styles, got {len(w)}")
    if any(not np.isfinite(x) or x < 0 for x in w):
        raise ValueError(f"style weights must be finite and >= 0, got {w}")
    total = sum(w)
    if total <= 0:
        raise ValueError("style weights must not all be zero")
    return [x / total for x in w]


@dataclass
class StyleBlend:
    """Style blending: a weighted set of StyleTargets, loss_s = sum_k w_k * style_loss(T_k, P).  The weights are normalised
    to sum to 1 here.  StepEngine runs a one-target blend exactly as its StyleTarget, a larger one in one call
    (strotss_step_losses_cw_fwd_bwd)."""
    targets: List[StyleTarget]
    weights: List[float]

    def __post_init__(self):
        self.targets = list(self.targets)
        if len(self.weights) != len(self.targets):
            raise ValueError(f"{len(self.targets)} style targets but {len(self.weights)} weights")
        self.weights = normalise_style_weights(self.weights)


STYLE_TRANSPORTS = ("remd", "sinkhorn", "sliced")
SINKHORN_MAX_ITERS = 64
DEFAULT_SINKHORN_L, DEFAULT_SINKHORN_ITERS = 10.0, 30
SINKHORN_LOG_MAX_L = 1000.0              # the log-domain entry's range: its f32 exponent carries 2 L 2^-24 of absolute error
SLICED_MAX_PROJECTIONS = 1024            # the library's range
DEFAULT_SLICED_PROJECTIONS = 256         # not tuned for image quality: a quarter of the range, 7 launches whatever the count


def check_style_transport(style_transport, sinkhorn_l, sinkhorn_iters, sliced_projections=DEFAULT_SLICED_PROJECTIONS,
                          sinkhorn_log=False) -> None:
    """ValueError unless the transport is a known one, sinkhorn_l finite and > 0, sinkhorn_iters a whole number in
    1..SINKHORN_MAX_ITERS and sliced_projections a whole number in 1..SLICED_MAX_PROJECTIONS (the library's ranges);
    sinkhorn_log goes with "sinkhorn" only, and with sinkhorn_l <= SINKHORN_LOG_MAX_L"""
    if style_transport not in STYLE_TRANSPORTS:
        raise ValueError(f"style_transport must be one of {STYLE_TRANSPORTS}, got {style_transport!r}")
    if isinstance(sinkhorn_l, bool) or not isinstance(sinkhorn_l, (int, float, np.integer, np.floating)) or \
            not np.isfinite(sinkhorn_l) or sinkhorn_l <= 0:
        raise ValueError(f"sinkhorn_l must be finite and > 0, got {sinkhorn_l!r}")
    if isinstance(sinkhorn_iters, bool) or not isinstance(sinkhorn_iters, (int, np.integer)) or \
            not 1 <= sinkhorn_iters <= SINKHORN_MAX_ITERS:
        raise ValueError(f"sinkhorn_iters must be a whole number in 1..{SINKHORN_MAX_ITERS}, got {sinkhorn_iters!r}")
    if isinstance(sliced_projections, bool) or not isinstance(sliced_projections, (int, np.integer)) or \
            not 1 <= sliced_projections <= SLICED_MAX_PROJECTIONS:
        raise ValueError(f"sliced_projections must be a whole number in 1..{SLICED_MAX_PROJECTIONS}, "
                         f"got {sliced_projections!r}")
    if not isinstance(sinkhorn_log, (bool, np.bool_)):
        raise ValueError(f"sinkhorn_log must be True or False, got {sinkhorn_log!r}")
    if sinkhorn_log and style_transport != "sinkhorn":
        raise ValueError(f"sinkhorn_log needs style_transport 'sinkhorn', got {style_transport!r}")
    if sinkhorn_log and sinkhorn_l > SINKHORN_LOG_MAX_L:
        raise ValueError(f"sinkhorn_l must be at most {SINKHORN_LOG_MAX_L:g} with sinkhorn_log, got {sinkhorn_l!r}")


PALETTE_TRANSPORTS = ("remd", "sliced")
PALETTE_MAX_PROJECTIONS = 1024           # the library's range
DEFAULT_PALETTE_PROJECTIONS = 64         # not tuned for image quality: the lattice estimates |v| to 1.5 % there


def check_palette_transport(palette_transport, palette_projections=DEFAULT_PALETTE_PROJECTIONS) -> None:
    """ValueError unless the palette transport is a known one and palette_projections a whole number in
    1..PALETTE_MAX_PROJECTIONS (the library's range)"""
    if palette_transport not in PALETTE_TRANSPORTS:
        raise ValueError(f"palette_transport must be one of {PALETTE_TRANSPORTS}, got {palette_transport!r}")
    if isinstance(palette_projections, bool) or not isinstance(palette_projections, (int, np.integer)) or \
            not 1 <= palette_projections <= PALETTE_MAX_PROJECTIONS:
        raise ValueError(f"palette_projections must be a whole number in 1..{PALETTE_MAX_PROJECTIONS}, "
                         f"got {palette_projections!r}")


def _require_one_gpu(what: str, strips, dist_group, plural: bool = False) -> None:
    """ValueError when an option that runs on one GPU (`what`; plural: "the ... run") meets image strips or region sharding"""
    if strips is not None or dist_group is not None:
        runs, it = ("run", "them") if plural else ("runs", "it")
        raise ValueError(f"{what} {runs} on one GPU: image strips and region sharding are not supported with {it}")


def extract_features(params: VGGParams, image: torch.Tensor) -> List[torch.Tensor]:
    """[image] + vgg(image)  (run_strotss.py:95-96), taps cloned out of a temporary trunk."""
    h, w = int(image.shape[1]), int(image.shape[2])
    trunk = VGGTrunk(params, h, w, with_grad=False)
    img = image.contiguous()
    return [img] + [t.clone() for t in trunk.forward(img)]


class _Capture:
    """`torch.cuda.graph(g)` without its gc.collect() + torch.cuda.empty_cache() (12 ms per capture, five captures per run:
    the step allocates nothing -- the warm-up has sized the engine's workspaces, which are frozen by now -- so there is no
    allocator state to tidy up before a capture).  The cyclic collector is held
    off while the stream captures: an earlier scale's engine is cyclic garbage (its stage lists hold bound methods), and a
    collection that lands inside the capture would run the destructors of its graphs and buffers -- runtime calls that a
    capturing stream does not allow -- at a moment that only the allocation count decides."""

    def __init__(self, graph: "torch.cuda.CUDAGraph", stream: "torch.cuda.Stream"):
        self.graph, self.stream = graph, stream

    def __enter__(self):
        torch.cuda.synchronize()
        self._gc = gc.isenabled()
        gc.disable()
        self._ctx = torch.cuda.stream(self.stream)
        self._ctx.__enter__()
        self.graph.capture_begin()
        return self

    def __exit__(self, *exc):
        try:
            if exc[0] is None:
                try:
                    self.graph.capture_end()
                finally:
                    self._ctx.__exit__(None, None, None)
                return False
            # the body raised: end the (now invalid) capture so the stream is usable again, but never let that second error
            # replace the one the caller has to see
            try:
                self.graph.capture_end()
            except Exception:
                pass
            self._ctx.__exit__(*exc)
            return False
        finally:
            if self._gc:
                gc.enable()


class StepEngine:
    """One scale of the coarse-to-fine loop: owns the 6 pyramid variables and their RMSprop slots.

    `regions` > 1 is the masked path (run_strotss.py:104-125): one trunk forward/backward, one
    index set + loss group per region, loss = mean over regions.  With `dist_group` (a ProcessGroup, or
    `parallel.WORLD` for torch.distributed's default group), regions are dealt round-robin to the ranks and the
    pixel gradient is all-reduced (sum) before the fold adjoint, so every rank applies the identical update.
    The logged scalars ride in the tail of the same buffer: ONE all-reduce per step.

    `content_weight`: an (h, w) or (1, h, w, 1) map at this scale's size, finite and >= 0 (strotss_utils.content_weight_at_scale
    builds it from a user's map): the content term of every region weights sample j's column of the self-similarity
    matrices by the map at sample j.  One GPU only: not with `strips` or `dist_group`.

    `temporal`, `detail`, `tv_weight`, `photo`: the pixel-space terms (nn/pixel_terms.py; DESIGN.md sections 12, 13, 26, 33) at
    this scale's size: a TemporalTarget or a sequence of 1..4 (certainties already combined, nearest frame first; one element
    is the TemporalTarget itself), a DetailTarget, the total variation's weight (0: no term), a PhotoTarget.  In that order
    their gradients join the pixel gradient after the trunk (and the all-reduce) and before the fold adjoint, once per step, not
    averaged over the regions; the bound terms there state the launches and what a weight of 0 does.  One GPU only, as the map.

    `style_transport`: "remd" (the relaxed EMD) or "sinkhorn" (DESIGN.md section 20): the entropic transport cost
    sinkhorn_knopp(target, prediction, 'cosine', sinkhorn_l, sinkhorn_iters) takes the place of the cosine relaxed EMD in
    every region and for every style of a blend, with its weight and in its scalar slot (l_remd); the moment, palette and
    content terms are unchanged.  One GPU only, as the map above.  "sliced" (DESIGN.md section 21): the sliced Wasserstein
    distance between the L2-normalised rows over `sliced_projections` sign directions stands there instead, in the same slot
    and with the same weight.  The directions of the engine's call number c (one call per region, style and step) are draw c
    of the Philox stream with key `sliced_seed` (rand.sliced_signs); the draw number lives in device memory, so a captured
    step draws fresh directions on every replay.  One GPU only.

    `sinkhorn_log` (with "sinkhorn" only): the same term with the scalings kept as logarithms, which
    stays a transport cost where exp(-sinkhorn_l * cost) underflows and the linear form's clamps act (it is guaranteed
    clamp-free only to sinkhorn_l = 13.8); sinkhorn_l up to SINKHORN_LOG_MAX_L.  False runs the linear form unchanged.

    `palette_transport`: "remd" (the palette relaxed EMD, the code it always ran, launch for launch) or "sliced" (DESIGN.md
    section 25): the sliced 1-Wasserstein distance between the YUV colours over `palette_projections` fixed directions
    (rand.palette_directions, one device buffer, the same on every step) stands where the palette relaxed EMD stands, for
    every region and every style of a blend, with the same weight and in the same scalar slot (l_palette, also returned as
    l_palette_sliced).  It conserves mass, which the relaxed EMD does not.  With "sliced" every `style_transport` takes the
    separate entries: with "remd" that is their 21 launches (19 with the new term's 2 in place of the palette relaxed EMD's
    4), not the grouped call's 13.  One GPU only."""

    N_SCALARS = 4   # loss_c, l_moment, l_remd, l_palette per region

    def __init__(self, params: VGGParams, content_feat: Sequence[torch.Tensor],
                 style_targets: Sequence[StyleTarget], stylized: torch.Tensor, alpha: float,
                 loss_denom: float, lr: float, sample_size: int = 1024, levels: int = 5,
                 dist_group=None, rho: float = 0.99, eps: float = 1e-8, strips: Optional["parallel.StripPlan"] = None,
                 deterministic: Optional[bool] = None, content_weight: Optional[torch.Tensor] = None,
                 temporal: Optional[Union[TemporalTarget, Sequence[TemporalTarget]]] = None,
                 style_transport: str = "remd", sinkhorn_l: float = DEFAULT_SINKHORN_L,
                 sinkhorn_iters: int = DEFAULT_SINKHORN_ITERS, sliced_projections: int = DEFAULT_SLICED_PROJECTIONS,
                 sliced_seed: int = 0, sinkhorn_log: bool = False, palette_transport: str = "remd",
                 palette_projections: int = DEFAULT_PALETTE_PROJECTIONS, detail: Optional[DetailTarget] = None,
                 tv_weight: float = 0.0, photo: Optional[PhotoTarget] = None):
        dev = stylized.device
        # the scratch memory of the losses and the trunk: the engine's own, so what its captured graphs point into lives and
        # dies with it and no other caller can regrow it (capture_graph freezes it)
        self._ws = _ops.Workspaces()
        check_palette_transport(palette_transport, palette_projections)
        check_style_transport(style_transport, sinkhorn_l, sinkhorn_iters, sliced_projections, sinkhorn_log)
        _check_prior_weight(tv_weight, "tv_weight")
        for chosen, what, plural in ((palette_transport == "sliced", "the sliced palette term", False),
                                     (style_transport == "sinkhorn", "the Sinkhorn style term", False),
                                     (style_transport == "sliced", "the sliced style term", False),
                                     (content_weight is not None, "a content-weight map", False),
                                     (temporal is not None, "the temporal term", False),
                                     (detail is not None or tv_weight > 0, "the pixel-space priors (detail, tv_weight)", True),
                                     (photo is not None, "the photorealism term", False)):
            if chosen:
                _require_one_gpu(what, strips, dist_group, plural)
        self.palette_transport, self.palette_projections = palette_transport, int(palette_projections)
        # the sliced palette term's directions: fixed for the life of the engine (a captured graph reads them at replay)
        self._palette_dirs = (torch.from_numpy(rand.palette_directions(self.palette_projections)).to(dev).contiguous()
                              if palette_transport == "sliced" else None)
        self.sinkhorn_log = bool(sinkhorn_log)
        self.style_transport, self.sinkhorn_l, self.sinkhorn_iters = style_transport, float(sinkhorn_l), int(sinkhorn_iters)
        self.sliced_projections, self.sliced_seed = int(sliced_projections), int(sliced_seed)
        # the sliced term's draw number: call number c of this engine uses draw c (the entry leaves it one higher)
        self._sliced_counter = torch.zeros(1, dtype=torch.int32, device=dev) if style_transport == "sliced" else None
        self.params = params
        self.alpha, self.loss_denom, self.lr, self.rho, self.eps = float(alpha), float(loss_denom), float(lr), rho, eps
        self.inv_alpha = 1.0 / max(self.alpha, 1.0)
        self.content_feat = [c.contiguous() for c in content_feat]
        # a one-target StyleBlend IS its target (same code path, bit for bit); larger blends: one region, no sharding
        self.style_targets = [t.targets[0] if isinstance(t, StyleBlend) and len(t.targets) == 1 else t for t in style_targets]
        self.R = len(self.style_targets)
        self._blended = any(isinstance(t, StyleBlend) for t in self.style_targets)
        if self._blended and (self.R > 1 or strips is not None or dist_group is not None):
            raise ValueError("style blending runs one region on one GPU: masks, image strips and region sharding are not "
                             "supported with several styles")
        h, w = self.h, self.w = int(stylized.shape[1]), int(stylized.shape[2])
        self._cw_map = None
        if content_weight is not None:
            self._cw_map = check_content_weight(content_weight, h, w).to(dev).clone()     # the engine's own copy
        # the pixel-space terms that are set, in the order they run and report; their zeroed workspaces are self._ws's
        self._pixel_terms = [term(arg, h, w, dev, self._ws) for term, arg, on in (
            (pixel_terms.TemporalTerm, temporal, temporal is not None), (pixel_terms.DetailTerm, detail, detail is not None),
            (pixel_terms.TVTerm, tv_weight, tv_weight > 0), (pixel_terms.PhotoTerm, photo, photo is not None)) if on]
        # --- variables = make_laplacian_pyramid(stylized) (run_strotss.py:89), rms slots start at 0
        self.variables = [v.contiguous() for v in make_laplacian_pyramid(stylized.contiguous(), levels)]
        self.rms = [torch.zeros_like(v) for v in self.variables]
        self.sizes = [(int(v.shape[1]), int(v.shape[2])) for v in self.variables]
        # fold temporaries: f[k] = v[k] + up(f[k+1]); f[0] is the image
        self.fold = [torch.empty_like(v) for v in self.variables[:-1]]
        self._fold_one_launch = None if os.environ.get("STROTSS_FOLD_ONE_LAUNCH", "1") != "0" else False
        # image strips (nn/parallel.py): the trunk covers rows [win0, win1) only; everything else is full-size
        self.strips = strips
        win0, win1 = (strips.win0, strips.win1) if strips is not None else (0, h)
        if strips is not None:
            assert strips.h == h, "image strips: plan made for this scale"
        # halo-exchange strips: the trunk refreshes its window's outermost rows from the neighbours after every layer
        self._halo = parallel.HaloExchange(strips, dist_group) if (strips is not None and strips.halo) else None
        self.trunk = VGGTrunk(params, win1 - win0, w, with_grad=True, halo=self._halo, ws=self._ws)
        # region sharding (masked runs): pixel gradient + the regions' scalars in ONE buffer = one all-reduce
        self.group = dist_group
        self.rank, self.world = parallel.world_info(dist_group) if dist_group is not None else (0, 1)
        self.my_regions = parallel.regions_for_rank(self.R, self.rank, self.world)
        # the sharded structure ([pixel gradient | scalars] in one buffer, graph | all-reduce | graph) also in a world of one
        # when STROTSS_DIST_FORCE=1 asks for it (the RCCL rehearsal on one GPU)
        self.sharded = dist_group is not None and (self.world > 1 or parallel.force_collectives())
        self._reduce_buf = None
        if self.sharded and strips is None:
            self._reduce_buf = torch.zeros(3 * h * w + self.R * 8, dtype=torch.float32, device=dev)
            self.trunk.gimg = self._reduce_buf[:3 * h * w].view(1, h, w, 3)
        self.d = 3 + sum(int(a.shape[-1]) for a in (self.trunk.acts[i] for i in self.trunk.taps))
        self.ld = _ops.pad32(self.d)
        rows = _ops.pad32(sample_size)
        self.sample_size = sample_size
        self.cf = [torch.zeros((rows, self.ld), dtype=torch.float32, device=dev) for _ in range(self.R)]
        # the regions' prediction rows are slices of ONE buffer: image strips all-reduce them in one collective
        self._pf_all = torch.zeros((self.R, rows, self.ld), dtype=torch.float32, device=dev)
        self.pf = [self._pf_all[r] for r in range(self.R)]
        self.gp = [torch.zeros((rows, self.ld), dtype=torch.float32, device=dev) for _ in range(self.R)]
        self.scalars = (torch.zeros((self.R, 8), dtype=torch.float32, device=dev) if self._reduce_buf is None
                        else self._reduce_buf[3 * h * w:].view(self.R, 8))
        # blended regions: the UNWEIGHTED moment / REMD / palette terms of every style (rows), losses() weighs them
        self._style_scalars = (torch.zeros((self.R, 3, _hip.MAX_STYLES), dtype=torch.float32, device=dev) if self._blended
                               else None)
        # every region's styles and weights, a StyleTarget as a one-style set of weight 1 (its own single-style launches in
        # the grouped call, its own floats in the separate entries); the grouped call's style set, None for a target
        # without x3 panels (separate entries only)
        self._styles = [(t.targets, t.weights) if isinstance(t, StyleBlend) else ([t], [1.0]) for t in self.style_targets]
        self._style_sets = [_ops.make_style_set(ts, ws) if len(ts) > 1 or ts[0].panels is not None else None
                            for ts, ws in self._styles]
        # the terms of a region, decided once: the grouped call stands for the relaxed EMDs only and needs a style set;
        # otherwise the separate entries with the style and the palette term of the engine's transports
        self._grouped_ok = [style_transport == "remd" and palette_transport == "remd" and s is not None
                            for s in self._style_sets]
        self._style_term, self._palette_term = self._choose_terms()
        # content-weight map: every region's weights of its samples (rows >= n zero), gathered with its features
        self._cw = self._mt_cw = None
        if self._cw_map is not None:
            self._cw = [torch.zeros(rows, dtype=torch.float32, device=dev) for _ in range(self.R)]
        # gradient of the variables: level 0 aliases the pixel gradient
        if strips is not None:
            # full-size pixel gradient, zero outside the window; the trunk writes its window rows in place
            self.gimg_full = torch.zeros((1, h, w, 3), dtype=torch.float32, device=dev)
            self.trunk.gimg = self.gimg_full[:, win0:win1]
            assert self.trunk.gimg.is_contiguous()
            self.gvars = [self.gimg_full] + [torch.empty_like(v) for v in self.variables[1:]]
        else:
            self.gvars = [self.trunk.gimg] + [torch.empty_like(v) for v in self.variables[1:]]
        # hypercolumn descriptors (pointers are static for the life of the engine)
        self._img_window = self.fold[0][:, win0:win1]
        self.pred_maps = [self._img_window] + [self.trunk.acts[i] for i in self.trunk.taps]
        gmaps = [self.trunk.gimg] + [self.trunk.grads[i] for i in self.trunk.taps]
        # divisors and clipping are those of the FULL maps (content_feat holds them), also for a window
        shapes = [_ops.hwc(m)[:2] for m in self.content_feat]
        self.divs = _ops.map_divisors(shapes)
        windows = None
        if strips is not None:
            windows = []
            for k, (m, (fh, _)) in enumerate(zip(self.pred_maps, shapes)):
                shift = (h // fh).bit_length() - 1 if fh < h else 0      # number of 2x2 pools above map k
                assert win0 % (1 << shift) == 0 and (win0 >> shift) + int(m.shape[1]) <= fh
                windows.append((win0 >> shift, fh))
        # (halo-exchange strips: the adjoint scatters ALL samples and drops the taps outside the window)
        self._mt_pred = _hip.make_maps(self.pred_maps, self.divs, gmaps, windows, window_drop=self._halo is not None)
        self._mt_content = _hip.make_maps(self.content_feat, self.divs)
        if self._cw_map is not None:
            self._mt_cw = _hip.make_maps([self._cw_map], [[]])        # level 0: the image's own coordinates, no divisors
        self._layer_to_map = {li: k + 1 for k, li in enumerate(self.trunk.taps)}
        self._layer_to_map[-1] = 0
        if strips is not None:            # strips shard the IMAGE: every rank runs every region's (replicated) losses
            self.my_regions, self.world = list(range(self.R)), 1
        self._ns = [0] * self.R
        # strips: the block [begin, end) of each region's (owner-ordered) samples this rank gathers and scatters lives in
        # DEVICE memory (strotss_maps_t.sample_range): it changes every step, a captured graph reads it at replay
        self._mt_pred_own = None
        if strips is not None:
            self._range_dev = torch.zeros((self.R, 2), dtype=torch.int32, device=dev)
            self._mt_pred_own = []
            for r in range(self.R):
                m = _hip.MapsT.from_buffer_copy(self._mt_pred)
                m.sample_range = self._range_dev[r].data_ptr()
                self._mt_pred_own.append(m)
        self._idx: List[Optional[torch.Tensor]] = [None] * self.R
        # deterministic mode (STROTSS_DETERMINISTIC=1): the tap adjoint as a sorted scatter, one plan per region and step
        # (no float atomics -> bitwise reproducible steps; the reference asks TF for the same: nn/rand.py:4-8)
        # default: off with a GPU to itself; ON when two ranks of the group sit on one card (parallel.ranks_share_a_gpu)
        env = os.environ.get("STROTSS_DETERMINISTIC")
        self.deterministic = bool(deterministic) if deterministic is not None else \
            (env == "1" if env is not None else parallel.ranks_share_a_gpu(dist_group))
        self._plans = None
        if self.deterministic:
            nb = _hip.lib().strotss_hypercol_scatter_plan_bytes(len(self.pred_maps))
            self._plans = [torch.empty(nb, dtype=torch.uint8, device=dev) for _ in range(self.R)]
        # bench.py's measurement hook (strotss_debug_winograd_stages) is process-wide: an engine must never be built, captured
        # or stepped under a partial stage mask, the convolutions would silently skip kernels
        if _hip.lib().strotss_debug_winograd_stages(7) != 7:
            raise _hip.StrotssHipError("strotss_debug_winograd_stages was left at a partial mask (a timing pass did not "
                                       "restore it): results since then are meaningless")
        self.steps_done = 0
        self._drawn_steps = 0             # the steps whose index sets the draw kernel made (draws_done)
        self._draw = None                 # device-side index draw (enable_device_draw): counters, masks, output buffers
        self._graph = None
        self._graph_post = None           # sharded regions: the part of the step after the all-reduce
        self._strip_graphs = None         # image strips: the three segments around the two all-reduces
        self._graph_drawn = False         # the captured graph starts with the draw kernel (no per-step upload)
        self._graph_idx: List[torch.Tensor] = []
        self._graph_n: List[int] = []

    # ------------------------------------------------------------------ pieces of the step
    def fold_forward(self) -> torch.Tensor:
        """img = fold_laplacian_pyramid(variables)   (strotss_utils.py:159-163)"""
        if self._fold_one_launch is not False:            # one launch for the whole fold (csrc/image.hip: fold_pyramid_kernel)
            if _ops.fold_pyramid(self.variables, self.fold[0]) is not None:
                self._fold_one_launch = True
                return self.fold[0]
            self._fold_one_launch = False                 # a pyramid shape the kernel does not take: level by level
        t = self.variables[-1]
        for k in range(len(self.variables) - 2, -1, -1):
            hk, wk = self.sizes[k]
            _ops.resize_bilinear(t, hk, wk, 1.0, self.variables[k], out=self.fold[k])
            t = self.fold[k]
        return self.fold[0]

    def _gather(self, maps_t, idx, out):
        n = idx.shape[0]
        _hip.check(_hip.lib().strotss_hypercol_gather(_hip.C.byref(maps_t), idx.data_ptr(), n, 1, out.data_ptr(),
                                                      self.ld, _hip.stream_ptr()), "hypercol_gather")

    def _gather_both(self, maps_pred, idx, r: int) -> None:
        """content rows, prediction rows and the zero fill of the gradient rows of region r in ONE launch (with a content-weight
        map also the weights of the samples)"""
        n = idx.shape[0]
        if self._cw is not None:
            _hip.check(_hip.lib().strotss_hypercol_gather2_cw(
                _hip.C.byref(self._mt_content), _hip.C.byref(maps_pred), _hip.C.byref(self._mt_cw), idx.data_ptr(), n, 1,
                self.cf[r].data_ptr(), self.pf[r].data_ptr(), self.ld, self.gp[r].data_ptr(), int(self.gp[r].shape[0]),
                self._cw[r].data_ptr(), int(self._cw[r].shape[0]), _hip.stream_ptr()), "hypercol_gather2_cw")
            return
        _hip.check(_hip.lib().strotss_hypercol_gather2(_hip.C.byref(self._mt_content), _hip.C.byref(maps_pred), idx.data_ptr(), n,
                                                       1, self.cf[r].data_ptr(), self.pf[r].data_ptr(), self.ld,
                                                       self.gp[r].data_ptr(), int(self.gp[r].shape[0]), _hip.stream_ptr()),
                   "hypercol_gather2")

    def _choose_terms(self):
        """The style term and the palette term of the separate entries, chosen once from the engine's transports: each is
        f(style target, pf, n, gscale, gp, out).  The relaxed EMD borrows the prediction rows' norms and x3 panels from the
        content loss's workspace (the moment term has its own) and the style rows' panels from the StyleTarget; so do the
        Sinkhorn and the sliced term.  Every term draws its scratch from the engine's workspaces, whose record of the content
        loss is therefore the engine's own."""
        ws = self._ws
        if self.style_transport == "sinkhorn":
            entry = _ops.sinkhorn_log_cos_fwd_bwd_after_selfsim if self.sinkhorn_log else _ops.sinkhorn_cos_fwd_bwd_after_selfsim

            def style_term(st, pf, n, g, gp, out):
                entry(st.feats, st.inv_norm, st.panels, st.ns, pf, n, self.d, self.sinkhorn_l, self.sinkhorn_iters, g, gp, out,
                      ws=ws)
        elif self.style_transport == "sliced":
            def style_term(st, pf, n, g, gp, out):
                _ops.sliced_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, st.ns, pf, n, self.d,
                                                      self.sliced_projections, self.sliced_seed, self._sliced_counter, g, gp, out,
                                                      ws=ws)
        else:
            def style_term(st, pf, n, g, gp, out):
                _ops.remd_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, st.ns, pf, n, self.d, g, gp, out, ws=ws)
        if self.palette_transport == "sliced":
            def palette_term(st, pf, n, g, gp, out):
                _ops.palette_sliced_fwd_bwd(st.feats, st.ns, pf, n, self._palette_dirs, g, gp, out, ws=ws)
        else:
            def palette_term(st, pf, n, g, gp, out):
                _ops.palette_remd_fwd_bwd(st.feats, st.ns, pf, n, g, gp, out, ws=ws)
        return style_term, palette_term

    def _losses(self, r: int, n: int, zeroed: bool = False):
        """(alpha*loss_c + loss_s)/loss_denom/R and its gradient w.r.t. the sampled prediction.  zeroed: the gradient rows
        were cleared by _gather_both already."""
        targets, weights = self._styles[r]
        pf, cf, gp, sc = self.pf[r], self.cf[r], self.gp[r], self.scalars[r]
        if n < pf.shape[0]:
            pf[n:].zero_(); cf[n:].zero_()
        if not zeroed:
            gp.zero_()
        base = 1.0 / (self.loss_denom * self.R)
        cw = self._cw[r] if self._cw is not None else None     # the samples' content weights (content-weight map)
        # moment / REMD / palette: the region's own scalars for one style, one unweighted value per style of a blend
        outs = (sc[1:], sc[2:], sc[3:]) if len(targets) == 1 else tuple(self._style_scalars[r])
        if self._grouped_ok[r] and _ops.step_losses_available():
            # one call: 13 launches instead of 21, the three forward GEMMs in one of them (bit for bit the separate entries
            # below for one style); a blend in as many launches
            _ops.step_losses_cw_fwd_bwd(pf, cf, n, self.d, cw, self._style_sets[r], self.alpha * base, base, base,
                                        self.inv_alpha * base, gp, sc[0:], *outs, ws=self._ws)
            return
        _ops.selfsim_weighted_fwd_bwd(pf, cf, cw, n, self.d, self.alpha * base, gp, sc[0:], ws=self._ws)
        for k, (st, w) in enumerate(zip(targets, weights)):
            _ops.moment_fwd_bwd(st.mean, st.cov, pf, n, self.d, base * w, gp, outs[0][k:], ws=self._ws)
            self._style_term(st, pf, n, base * w, gp, outs[1][k:])
            self._palette_term(st, pf, n, self.inv_alpha * base * w, gp, outs[2][k:])

    def _scatter_maps(self, r: int):
        """descriptor + sample count of region r's tap adjoint: strips (recompute margin) = this rank's block of the samples
        (device-side range); halo-exchange strips = every sample, taps outside the window dropped; otherwise all samples."""
        if self.strips is not None and self._halo is None:
            return self._mt_pred_own[r], self._ns[r]
        if self.strips is not None:
            return self._mt_pred, self._ns[r]
        return self._mt_pred, int(self._idx[r].shape[0])

    def _scatter(self, layer_index: int, k_end: Optional[int] = None):
        k = self._layer_to_map[layer_index]
        k_end = k + 1 if k_end is None else k_end
        for r in self.my_regions:
            mt, n = self._scatter_maps(r)
            idx, gp = self._idx[r][:n], self.gp[r][:n]
            if self.deterministic:
                _ops.hypercol_scatter_sorted(mt, self._plans[r], n, gp, relu_mask_from=1, map_begin=k, map_end=k_end)
            else:
                _ops.hypercol_scatter(self.pred_maps, None, idx, gp, relu_mask_from=1, map_begin=k, map_end=k_end, maps_t=mt)

    def _scatter_all(self):
        """every map's taps in one launch per region (pre-scatter backward of the small scales, nn/model.py)"""
        self._scatter(-1, len(self.pred_maps))

    # ------------------------------------------------------------------ the step as one stage list
    def _stages(self, indices: Optional[Sequence[torch.Tensor]], apply: bool = True):
        """The step as [(device segment, host collective after it or None)], a segment a list of calls: what the eager step
        runs, capture_graph captures (one graph per segment) and a replay interleaves with the same collectives.
            plain            [pixel gradient, pixel terms, fold adjoint]
            region-sharded   [pixel gradient] | all-reduce _reduce_buf | [pixel terms, fold adjoint]
            image strips     [_strip_stage_a] | all-reduce _pf_all | [_strip_stage_b] | all-reduce gimg_full | [fold adjoint]
        apply: apply_gradients ends the last segment.  indices: the index sets of the pixel gradient, None = the draw kernel
        at the head of the step (image strips: the sets _strip_inputs has put in place)."""
        end = [self._fold_adjoint] + ([self.apply_gradients] if apply else [])
        if self.strips is not None:
            # the rows of the other ranks' samples arrive in _pf_all; the windows overlap by the margins: sum gimg_full
            return [([self._strip_stage_a], lambda: parallel.allreduce_sum_(self._pf_all, self.group)),
                    ([self._strip_stage_b], lambda: parallel.allreduce_sum_(self.gimg_full, self.group)),
                    (end, None)]
        head = [lambda: self._pixel_gradient(self._draw_indices() if indices is None else indices)]
        tail = [self._run_pixel_terms] + end
        return [(head, self._reduce), (tail, None)] if self.sharded else [(head + tail, None)]

    @staticmethod
    def _run(stages) -> None:
        for segment, collective in stages:
            for call in segment:
                call()
            if collective is not None:
                collective()

    def _inputs(self, indices: Optional[Sequence[torch.Tensor]], strip_offsets, static: bool):
        """The host side of a step, ahead of its stage list: the index sets copied into the captured graphs' static buffers
        (static) and, with image strips, this rank's block of every set (_strip_inputs).  Returns the sets the stages read."""
        if indices is None:                  # drawn on the device, inside the step
            return None
        assert len(indices) == self.R
        if static:
            for dst, src in zip(self._graph_idx, indices):
                dst.copy_(src, non_blocking=True)
            indices = self._graph_idx
        if self.strips is not None:
            self._strip_inputs(indices, strip_offsets)
        return indices

    def forward_backward(self, indices: Sequence[torch.Tensor], strip_offsets: Optional[Sequence[int]] = None) -> None:
        """train_step (run_strotss.py:131-142 / 104-125): fills self.gvars and self.scalars.
        With image strips every region's `indices[r]` must be ordered by owning rank and `strip_offsets[r]` be its world + 1
        block offsets (parallel.sort_indices_by_strip); one region: the offsets list itself is accepted too."""
        self._run(self._stages(self._inputs(indices, strip_offsets, static=False), apply=False))

    def _pixel_gradient(self, indices: Sequence[torch.Tensor]) -> None:
        """fold, trunk forward, this rank's regions' samples + losses, trunk data-gradient -> trunk.gimg, scalars"""
        if self.sharded:
            self.scalars.zero_()          # regions owned by other ranks arrive through the all-reduce
        img = self.fold_forward()
        self.trunk.forward(img)
        for r in self.my_regions:
            idx = _hip.require(indices[r], "indices")
            n = int(idx.shape[0])
            assert 0 < n <= self.sample_size and idx.shape[1] == 2
            self._idx[r] = idx
            self._gather_both(self._mt_pred, idx, r)
            if self.deterministic:
                _ops.hypercol_scatter_plan(self._mt_pred, idx, self._plans[r])
            self._losses(r, n, zeroed=True)
        if self.my_regions:
            self.trunk.backward(self._scatter, self._scatter_all)
        else:
            self.trunk.gimg.zero_()

    def _reduce(self) -> None:
        """sharded regions: ONE all-reduce(sum) over [pixel gradient | scalars] (RCCL over xGMI; 12 MiB at 1024^2)"""
        if self._reduce_buf is not None:
            parallel.allreduce_sum_(self._reduce_buf, self.group)

    def _run_pixel_terms(self) -> None:
        """gvars[0] += weight * dL/dx and the scalars of every pixel-space term in turn, x the folded image of this step"""
        for term in self._pixel_terms:
            term.run(self.fold[0], self.gvars[0])

    def _fold_adjoint(self) -> None:
        """gvars[k] = up^T(gvars[k-1]): adjoint of the fold"""
        if self._fold_one_launch is not False and _ops.fold_pyramid_adjoint(self.gvars):     # two levels per launch
            return
        for k in range(1, len(self.variables)):
            hk, wk = self.sizes[k]
            _ops.resize_bilinear_adjoint(self.gvars[k - 1], hk, wk, out=self.gvars[k])

    # ---- image strips: the step in three stages with an all-reduce between them
    def _strip_inputs(self, indices: Sequence[torch.Tensor], offsets) -> None:
        """Host side of a strips step (never captured): every region's index set (ordered by owning rank) and this rank's
        block of it, the block bounds going to device memory."""
        if self.R == 1 and offsets is not None and not isinstance(offsets[0], (list, tuple)):
            offsets = [offsets]
        assert offsets is not None and len(offsets) == self.R
        bounds = []
        for r in range(self.R):
            idx = _hip.require(indices[r], "indices")
            n = int(idx.shape[0])
            off = offsets[r]
            assert len(off) == self.strips.world + 1 and off[-1] == n
            assert 0 < n <= self.sample_size and idx.shape[1] == 2
            self._idx[r], self._ns[r] = idx, n
            bounds.append((int(off[self.strips.rank]), int(off[self.strips.rank + 1])))
        # a fresh pinned block per step (the caching host allocator hands it out again only after this copy has run: the
        # host may be several steps ahead of the GPU)
        host = torch.tensor(bounds, dtype=torch.int32)
        self._range_dev.copy_(host.pin_memory() if self._range_dev.is_cuda else host, non_blocking=True)

    def _strip_stage_a(self, indices=None, offsets=None) -> None:
        """fold (replicated), trunk forward on the window; per region: content rows (all, from the replicated full maps),
        prediction rows of THIS rank's samples (the others stay zero for the all-reduce).  Capturable: nothing here
        depends on the block bounds on the host.  (indices, offsets given: _strip_inputs first -- the eager form.)"""
        if indices is not None:
            self._strip_inputs(indices, offsets)
        self.fold_forward()
        self.trunk.forward(self._img_window)
        self._pf_all.zero_()
        for r in range(self.R):
            idx = self._idx[r]
            self._gather_both(self._mt_pred_own[r], idx, r)

    def _strip_stage_b(self) -> None:
        """losses of every region on the assembled features (replicated), backward of this rank's rows through its window."""
        for r in range(self.R):
            self._losses(r, self._ns[r], zeroed=True)
        if self.deterministic:
            for r in range(self.R):
                mt, n = self._scatter_maps(r)
                _ops.hypercol_scatter_plan(mt, self._idx[r][:n], self._plans[r])
        if self._halo is not None:
            # every rank back-propagates (gradient crosses the strip borders through the exchanges, and every sample's
            # taps that land in this window are scattered here); only the OWN rows of the pixel gradient are kept
            self.trunk.backward(self._scatter)
            self.gimg_full[:, :self.strips.own0].zero_()
            self.gimg_full[:, self.strips.own1:].zero_()
            return
        self.trunk.backward(self._scatter, self._scatter_all)     # (a rank without samples back-propagates zeros)
        # rows outside the window still hold the previous step's all-reduced sum
        self.gimg_full[:, :self.strips.win0].zero_()
        self.gimg_full[:, self.strips.win1:].zero_()

    # ---- the step's sample coordinates drawn on the device (csrc/draw.hip), inside the step and inside its graph
    def enable_device_draw(self, seed: int, t0: int = 0, masks: Optional[Sequence] = None, sample_levels=None) -> bool:
        """Draw every step's index sets on the device (reference: Sampling._make_indices inside the traced train_step,
        strotss_utils.py:83-121 / run_strotss.py:136, 115): region r of step s uses draw number t0 + s*R + r of the Philox
        stream with key `seed` -- what `make_indices_np(..., rng=rand.PhiloxStream(seed, t0))` called region by region, step
        by step, returns on the host.  masks: per region a boolean (h, w) host array at this scale, or None.
        sample_levels (--sample_map): one (h, w) uint16 host array of importance levels used for every
        region, or a per-region list (None: that region draws uniformly); the draw is then strotss_index_draw_weighted and
        `make_indices_weighted_np` its host twin.
        Returns False (and changes nothing) where the device draw does not apply: image strips (the host orders every set
        by owning rank), a grid of more than 32768 candidates, or a region that an unlucky offset leaves with fewer
        candidates than samples (the sample count must be the same at every step: it shapes the launches)."""
        if self.strips is not None:
            return False
        masks = list(masks) if masks is not None else [None] * self.R
        assert len(masks) == self.R
        most, least = _ops.index_draw_counts(self.h, self.w, masks)
        if most > 32768 or least < self.sample_size or self.R > _hip.MAX_DRAW_REGIONS or self.sample_size > 1024:
            return False
        dev = self.variables[0].device
        counters = torch.tensor([int(t0) + r for r in range(self.R)], dtype=torch.int64).to(torch.int32).to(dev)
        mask_dev = [None if m is None else torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint8)).to(dev) for m in masks]
        idx = [torch.zeros((self.sample_size, 2), dtype=torch.float32, device=dev) for _ in range(self.R)]
        levels = None
        if sample_levels is not None:
            per_region = list(sample_levels) if isinstance(sample_levels, (list, tuple)) else [sample_levels] * self.R
            assert len(per_region) == self.R
            shared = {}                          # one device copy of a map that several regions use
            for q in per_region:
                if q is not None and id(q) not in shared:
                    a = np.ascontiguousarray(q)
                    if a.dtype != np.uint16 or a.shape != (self.h, self.w):
                        raise ValueError(f"sample levels of dtype {a.dtype} and shape {a.shape}: expected uint16 "
                                         f"({self.h}, {self.w})")
                    shared[id(q)] = torch.from_numpy(a).to(dev)
            levels = [None if q is None else shared[id(q)] for q in per_region]
        self._draw = dict(seed=int(seed), t0=int(t0), counters=counters, masks=mask_dev, idx=idx, levels=levels)
        return True

    def draws_done(self) -> int:
        """draws consumed so far by the device stream (to advance the host twin: rand.PhiloxStream.skip)"""
        return self._drawn_steps * self.R

    def _draw_indices(self) -> List[torch.Tensor]:
        dr = self._draw
        if dr["levels"] is not None:
            _ops.index_draw_weighted(self.h, self.w, self.sample_size, dr["seed"], dr["counters"], dr["idx"], dr["levels"],
                                     dr["masks"])
        else:
            _ops.index_draw(self.h, self.w, self.sample_size, dr["seed"], dr["counters"], dr["idx"], dr["masks"])
        return dr["idx"]

    def apply_gradients(self) -> None:
        """opt.apply_gradients (run_strotss.py:148): Keras RMSprop, all 6 tensors in one launch."""
        _ops.rmsprop_step(self.variables, self.rms, self.gvars, self.lr, self.rho, self.eps)

    def step(self, indices: Optional[Sequence[torch.Tensor]] = None, strip_offsets: Optional[Sequence[int]] = None) -> None:
        """One optimisation step.  indices None: the index sets are drawn on the device at the head of the step
        (enable_device_draw first); otherwise they are the caller's (injected: tests, fixtures, strips)."""
        drawn = indices is None
        assert not drawn or self._draw is not None, "step() without indices needs enable_device_draw()"
        graphs = self._captured()
        if graphs is not None and drawn == self._graph_drawn and \
                (drawn or all(int(i.shape[0]) == n for i, n in zip(indices, self._graph_n))):
            self._inputs(indices, strip_offsets, static=True)
            for g, (_, collective) in zip(graphs, self._stages(None)):
                g.replay()
                if collective is not None:
                    collective()
        else:                                # eager (also a step whose index counts differ from the captured ones)
            self._run(self._stages(self._inputs(indices, strip_offsets, static=False)))
        self.steps_done += 1
        self._drawn_steps += drawn

    def _captured(self):
        """the captured graphs, one per segment of _stages, or None: the step runs eagerly"""
        if self.strips is not None:
            return self._strip_graphs
        if self._graph is None:
            return None
        return (self._graph,) if self._graph_post is None else (self._graph, self._graph_post)

    def capture_graph(self, example_indices: Optional[Sequence[torch.Tensor]] = None, example_offsets=None) -> None:
        """Capture the step (_stages: forward_backward + apply_gradients) into hipGraphs, one per device segment (the ~100
        launches of a step replay as one submission; the 64-256 px scales are otherwise bound by host launch rate).  Index
        sets are copied into static buffers before each replay; a step whose index counts differ from the captured ones runs
        eagerly.  The captured step does not advance the optimisation: the variables / RMSprop slots (and the draw counters)
        are snapshotted around the warm-up and capture passes; the warm-up is one whole eager step, collectives included.
        It sizes the engine's own workspaces (self._ws), which are then frozen: the graphs point into memory that belongs to
        this engine, that no other caller can regrow and that a later eager step of the engine's may not reallocate either.
        Sharded regions (world > 1): TWO graphs, [fold .. pixel gradient] and [pixel terms + fold adjoint + RMSprop], the
        all-reduce launched between their replays.  Image strips (recompute margin; example_offsets = the block offsets of
        example_indices): THREE graphs, [fold .. gathers], [losses .. pixel gradient of the window], [fold adjoint + RMSprop],
        the two all-reduces between their replays; the block of samples a rank owns changes every step and is read from
        device memory (strotss_maps_t.sample_range).  Halo-exchange strips run eagerly (their trunk exchanges rows from Python
        after every layer)."""
        if self.strips is not None and (self._halo is not None or example_offsets is None):
            return
        drawn = example_indices is None        # the draw kernel is the first node of the graph: nothing to upload per step
        state = self.variables + self.rms
        if self._sliced_counter is not None:
            state = state + [self._sliced_counter]         # the sliced term's draw number: likewise put back
        if drawn:
            assert self._draw is not None, "capture_graph() without indices needs enable_device_draw()"
            state = state + [self._draw["counters"]]       # warm-up and capture passes draw too: put the counters back
            self._graph_idx = self._draw["idx"]
            self._graph_n = [self.sample_size] * self.R
        else:
            self._graph_idx = [i.clone() for i in example_indices]
            self._graph_n = [int(i.shape[0]) for i in example_indices]
        snap = [t.clone() for t in state]
        stages = self._stages(None if drawn else self._inputs(self._graph_idx, example_offsets, static=False))
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):              # warm-up on the side stream: workspaces, collectives, library state
            if any(n < self.sample_size for n in self._graph_n):
                # a later step with other index counts runs eagerly and may bring more samples than the captured one: the
                # loss workspaces take the size of the largest set first (on whatever the rows hold; the warm-up overwrites it)
                for r in self.my_regions:
                    self._losses(r, self.sample_size)
            self._run(stages)
        # the warm-up has sized the engine's workspaces.  What protects the graphs from here on is ownership plus this freeze:
        # nobody else draws from self._ws, and a request of the engine's own that would reallocate a buffer raises
        self._ws.freeze()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graphs = []
        for segment, _ in stages:
            graphs.append(torch.cuda.CUDAGraph())
            with _Capture(graphs[-1], side):
                for call in segment:
                    call()
        for t, s0 in zip(state, snap):
            t.copy_(s0)
        if self.strips is not None:
            self._strip_graphs = tuple(graphs)
        else:
            self._graph, self._graph_post, self._graph_drawn = graphs[0], (graphs[1] if len(graphs) > 1 else None), drawn

    # ------------------------------------------------------------------ read-outs (host sync)
    def losses(self) -> dict:
        s = self.scalars.detach().cpu().numpy().astype(np.float64)
        per_style = None
        if self._blended:
            # blended regions: the three style terms are the weighted sums of the per-style (unweighted) ones
            terms = self._style_scalars.detach().cpu().numpy().astype(np.float64)
            per_style = []
            for r, t in enumerate(self.style_targets):
                if not isinstance(t, StyleBlend):
                    continue
                w = np.asarray(t.weights, dtype=np.float64)
                k = len(w)
                s[r, 1:4] = terms[r, :, :k] @ w
                per_style = [{"weight": float(w[i]), "l_moment": float(terms[r, 0, i]), "l_remd": float(terms[r, 1, i]),
                              "l_palette": float(terms[r, 2, i]),
                              "loss_s": float(terms[r, 0, i] + terms[r, 1, i] + self.inv_alpha * terms[r, 2, i])}
                             for i in range(k)]
        lc = s[:, 0]
        ls = s[:, 1] + s[:, 2] + self.inv_alpha * s[:, 3]
        loss = ((self.alpha * lc + ls) / self.loss_denom).mean()
        out = {"loss": float(loss), "loss_c": float(lc.mean()), "loss_s": float(ls.mean()),
               "l_moment": float(s[:, 1].mean()), "l_remd": float(s[:, 2].mean()),
               "l_palette": float(s[:, 3].mean())}
        if self.style_transport == "sinkhorn":    # the slot of l_remd holds the Sinkhorn term: also under its own name
            out["l_sinkhorn"] = out["l_remd"]
        if self.style_transport == "sliced":      # likewise the sliced term
            out["l_sliced"] = out["l_remd"]
        if self.palette_transport == "sliced":    # the slot of l_palette holds the sliced palette term
            out["l_palette_sliced"] = out["l_palette"]
        if per_style is not None:
            out["per_style"] = per_style         # one dict per style of the blend: its weight and unweighted terms
        for term in self._pixel_terms:           # once per step, not averaged over the regions; added in the list's order
            out["loss"] = out["loss"] + term.report(out)
        return out

    def stylized(self) -> torch.Tensor:
        return self.fold_forward().clone()


# -------------------------------------------------------------------------------------------
def smoke_check(O, np_, torch_) -> None:
    """__graft_entry__.smoke(): one tiny optimisation step on cuda:0 checked against the oracle."""
    from .model import synthetic_weights
    dev = torch_.device("cuda", 0)
    torch_.cuda.set_device(dev)
    g = torch_.Generator().manual_seed(0)
    content = torch_.rand(1, 32, 32, 3, generator=g, dtype=torch_.float32)
    style = torch_.rand(1, 32, 32, 3, generator=g, dtype=torch_.float32)
    weights = synthetic_weights('16', 0)
    rng = np_.random.default_rng(0)
    s_idx = O.make_indices(32, 32, False, 256, rng)
    idx = O.make_indices(32, 32, True, 256, rng)
    alpha, denom, lr = 16.0, 18.0625, 2e-3
    # oracle (float64)
    vgg = O.VGG(weights, dtype=torch_.float64)
    c64, s64 = content.double(), style.double()
    with torch_.no_grad():
        cf = [c64] + vgg(c64); sf = [s64] + vgg(s64)
        ss = O.sample_features(sf, s_idx, False)
    init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]
    ref = O.train_step(variables, vgg, cf, ss, idx, alpha, denom)
    # HIP
    params = VGGParams(weights, '16', None, dev)
    cfeat = extract_features(params, content.to(dev))
    sfeat = extract_features(params, style.to(dev))
    sfe = _ops.hypercol_gather(sfeat, torch_.from_numpy(s_idx).to(dev), False)
    st = StyleTarget.build(sfe, s_idx.shape[0], 2179)
    eng = StepEngine(params, cfeat, [st], init.float().to(dev), alpha, denom, lr, sample_size=256)
    eng.step([torch_.from_numpy(idx).to(dev)])
    torch_.cuda.synchronize()
    got = eng.losses()
    assert abs(got["loss"] - float(ref["loss"])) < 1e-4 * max(1.0, abs(float(ref["loss"]))), (got, float(ref["loss"]))
    g0 = eng.gvars[0].cpu().double()
    rel = float((g0 - ref["grads"][0]).norm() / ref["grads"][0].norm())
    assert rel < 2e-2, rel
    print(f"smoke ok: loss {got['loss']:.6f} (oracle {float(ref['loss']):.6f}), pixel-grad rel err {rel:.2e}")
